"""CPU-side checks: the C-ABI library loads and exports every symbol the header declares, the
product modules reproduce the reference's state_dict contract, host-side control utilities behave
like the reference's, and the product refuses to run without a GPU (there is no CPU fallback)."""
import os
import random
import re

import pytest
import torch

from conftest import REPO
from adaptive_stereo import _native as nat
from adaptive_stereo.models.stereo_net import StereoNet, FeatureExtractorNetwork
from adaptive_stereo.utils.ema import online_ema
from adaptive_stereo.utils.stereo_reservoir import StereoReservoir

HEADER = os.path.join(REPO, "include", "adaptive_stereo_hip.h")


def declared_symbols():
  text = open(HEADER).read()
  text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
  return sorted(set(re.findall(r"\b(as_[a-z0-9_]+)\s*\(", text)))


def test_library_loads_and_exports_every_declared_symbol():
  lib = nat.load()
  names = declared_symbols()
  assert len(names) >= 30
  for n in names:
    assert hasattr(lib, n), "libadaptive_stereo_hip.so does not export %s" % n
  # the ctypes signature table covers exactly the header
  assert sorted(nat.EXPORTED_SYMBOLS) == names
  assert lib.as_version() >= 1


def test_geometry_helpers_without_gpu():
  lib = nat.load()
  g = nat.Pcl(2, 12, 24, 78, 1, 1, 1)
  assert lib.as_pcl_numel(g) == 2 * 14 * 26 * 80 * 32 == g.numel()
  assert lib.as_conv32_num_blocks(g) == (2 * 12 * 24 * 78 + 127) // 128
  s = nat.ConvShape(3, 3, 3, 1, 1, 1, 1, 1)
  assert lib.as_conv32_wgrad_workspace(g, g, s) > 0
  # argument validation happens before any launch
  bad = nat.Pcl(0, 1, 1, 1, 0, 0, 0)
  assert lib.as_cost_volume_fwd(None, None, None, bad, None) != 0
  assert b"geometry" in lib.as_last_error()


@pytest.mark.parametrize("k", [3, 4])
def test_state_dict_contract_matches_reference(k, golden_loader):
  """Key names, shapes and dtypes equal the reference's (taken from the fixtures' 'after/' entries,
  which were dumped from the reference's own state_dict())."""
  gold = golden_loader("plumbing_240x320_k3_b1" if k == 3 else "crop_96x256_k4_b1")
  fnet, snet = FeatureExtractorNetwork(k), StereoNet(k, 1, 0, maxdisp=192)
  for prefix, net, expect in (("stereo", snet, 123), ("feature", fnet, 92 if k == 3 else 94)):
    sd = net.state_dict()
    assert len(sd) == expect
    ref_keys = sorted(x[len("after/%s." % prefix):] for x in gold.z.files if x.startswith("after/%s." % prefix))
    ref_keys += sorted(x[len("shape__after/%s." % prefix):] for x in gold.z.files
                       if x.startswith("shape__after/%s." % prefix))
    assert sorted(sd.keys()) == sorted(set(ref_keys))
    for name, t in sd.items():
      skey = "shape__after/%s.%s" % (prefix, name)
      if skey in gold.z.files:
        assert tuple(t.shape) == tuple(int(v) for v in gold.z[skey]), name
  assert snet.state_dict()["filter.0.0.0.weight"].shape == (32, 32, 3, 3, 3)
  assert "edge_aware_refinements.0.residual_astrous_blocks.3.conv2.1.running_var" in snet.state_dict()


def test_product_refuses_cpu_tensors():
  fnet, snet = FeatureExtractorNetwork(3), StereoNet(3, 1, 0, maxdisp=64)
  x = torch.zeros(1, 3, 32, 32)
  with pytest.raises(RuntimeError, match="no CPU path"):
    fnet(x)
  with pytest.raises(RuntimeError, match="no CPU path"):
    snet(x, torch.zeros(1, 32, 4, 4), torch.zeros(1, 32, 4, 4), "l")


def test_shared_refusals_of_the_device_side_operators():
  from adaptive_stereo import collect
  with pytest.raises(RuntimeError, match=r"adaptive_stereo: Thing lives on the GPU \(got cpu\); there is no CPU path"):
    collect.gpu_device("Thing", "cpu")
  assert collect.gpu_device("Thing", "cuda:1") == torch.device("cuda:1")
  cpu, code = torch.device("cpu"), torch.zeros(2, 1, 3, 8, dtype=torch.uint8)
  collect.check_u8("op", "code", code, (2, 1, 3, 8), cpu)
  for bad in (code.float(), code[..., ::2], code[:, :, :, :4].contiguous(), None):
    with pytest.raises(RuntimeError, match=r"op: code must be a contiguous uint8 \(2, 1, 3, 8\) tensor on cpu \(got "):
      collect.check_u8("op", "code", bad, (2, 1, 3, 8), cpu)
  with pytest.raises(RuntimeError, match=r"op: x must be \(2, 1, 3, 8\) on cpu \(got \(2, 1, 3, 4\) on cpu\)"):
    collect.check_shape("op", "x", torch.zeros(2, 1, 3, 4), (2, 1, 3, 8), cpu)
  for size in ((0, 4, 1), (4, 4, 0)):
    with pytest.raises(ValueError, match="MapOperator: size %d x 4, batch %d" % (size[0], size[2])):
      collect.MapOperator(*size, device="cuda")
  with pytest.raises(RuntimeError, match="no CPU path"):
    collect.MapOperator(4, 4, 1, device="cpu")


def test_parameter_gradients_go_to_both_sinks_or_to_two_fresh_tensors():
  """hip_ops._grad_dest decides for every backward kernel with a (weight, bias)-like gradient pair: both sinks and
  accumulate = 1, or two fresh tensors and accumulate = 0, never one of each; hip_ops._rmw records nothing outside a
  multi-stream region."""
  from adaptive_stereo import hip_ops
  sw, sb = torch.zeros(32, 4, 3, 3), torch.zeros(32)
  dev = sw.device
  w, b, acc = hip_ops._grad_dest(sw, sb, sw.shape, sb.shape, dev)
  assert w is sw and b is sb and acc == 1
  for sink_w, sink_b in ((None, sb), (sw, None), (None, None)):
    w, b, acc = hip_ops._grad_dest(sink_w, sink_b, (32, 4, 3, 3), (32,), dev)
    assert acc == 0
    assert w.shape == sw.shape and b.shape == sb.shape and w.dtype == b.dtype == torch.float32
    assert w.is_contiguous() and b.is_contiguous()
    for fresh in (w, b):
      assert all(fresh.data_ptr() != s.data_ptr() for s in (sw, sb))
  # a layer without bias: the weight's sink alone decides, and there is no bias gradient either way
  w, b, acc = hip_ops._grad_dest(sw, None, sw.shape, None, dev)
  assert w is sw and b is None and acc == 1
  w, b, acc = hip_ops._grad_dest(sw, sb, sw.shape, None, dev)
  assert w is sw and b is None and acc == 1
  w, b, acc = hip_ops._grad_dest(None, sb, sw.shape, None, dev)
  assert w.shape == sw.shape and w.data_ptr() != sw.data_ptr() and b is None and acc == 0
  # ordering: nothing is recorded for None, and nothing while no multi-stream region is open
  assert hip_ops._RmwOrder.enabled is False and hip_ops._RmwOrder.last == {}
  ran = []
  with hip_ops._rmw(None):
    ran.append(1)
  with hip_ops._rmw(sw):
    ran.append(2)
  assert ran == [1, 2]
  assert hip_ops._RmwOrder.last == {} and hip_ops._RmwOrder.streams == {}


def test_reservoir_is_uniform_like_the_reference():
  """Mirrors the reference's test/test_stereo_reservoir.py: mean of kept items ~ 500 +- 5."""
  random.seed(123)
  total = 0.0
  trials = 1000
  for _ in range(trials):
    r = StereoReservoir(10)
    for i in range(1000):
      r.add(None, None, float(i), i)
    assert r.size() == 10
    total += r.average_value()
  assert abs(total / trials - 499.5) < 5.0
  r = StereoReservoir(2)
  assert r.add(None, None, 1.0, 7) is True
  assert r.add(None, None, 1.0, 7) is False          # duplicate index refused
  r.update_value(0, 3.0)
  assert r.average_value() == 3.0


def test_online_ema():
  assert online_ema(2.0, 4.0, weight=0.75) == 2.0 * 0.75 + 0.25 * 4.0
  t = online_ema(torch.tensor(1.0), torch.tensor(3.0))
  assert abs(float(t) - (0.999 + 0.003)) < 1e-6


def test_division_by_9_and_3_in_three_instructions_is_correctly_rounded(tmp_path):
  """photometric.hip divides by 9 and 3 as q = x*c, r = fma(-q, y, x), q' = fma(r, c, q).  The claim — equal to the IEEE
  quotient for every finite binary32 x except -0 — is checked by tests/tools/div_const.c (all 2^32 patterns when run by
  hand; here every 61st, ~70 million, with the host's hardware fma)."""
  import shutil, subprocess
  if shutil.which("gcc") is None:
    pytest.skip("no gcc")
  src = os.path.join(REPO, "tests", "tools", "div_const.c")
  exe = str(tmp_path / "div_const")
  subprocess.run(["gcc", "-O2", "-mfma", "-fopenmp", "-ffp-contract=off", "-DSTRIDE=61", src, "-o", exe, "-lm"], check=True)
  out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
  assert out.returncode == 0, out.stdout + out.stderr


def test_hand_waited_loads_are_never_read_in_flight():
  """The kernels that issue global loads from inline asm and retire them with their own s_waitcnt must not let hipcc read (copy,
  spill) a destination register between the load and its wait: tests/tools/check_async_loads.py compiles them to gfx950 ISA and
  scans for such reads (found once: ten v_mov in front of a branch that held two different waits — stale operands that came and
  went with memory latency, different from process to process)."""
  import shutil, subprocess, sys
  if not (os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("hipcc")):
    pytest.skip("no hipcc")
  tool = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools", "check_async_loads.py")
  r = subprocess.run([sys.executable, tool], capture_output=True, text=True, timeout=900)
  assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
  assert "conv32_wino_kernel" in r.stdout and "HAZARD" not in r.stdout
  # the matrix-pipe hazards around inline-asm vector instructions (round 4: the packed differences of conv32_wino_dev.h): the
  # scan must FLAG the build without the hazard guards — the build that made two launches of one kernel differ
  env = dict(os.environ, CHECK_EXTRA_FLAGS="-DWN_TEST_NO_HAZARD_GUARD")
  wino = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "adaptive-stereo-icra-2021_amd", "csrc", "conv32_wino.hip")
  r2 = subprocess.run([sys.executable, tool, wino], capture_output=True, text=True, timeout=900, env=env)
  assert r2.returncode == 1 and "MATRIX-PIPE DATA HAZARD" in r2.stdout, r2.stdout[-2000:]


def test_every_tile_of_the_3d_weight_gradient_is_covered_three_times():
  """csrc/conv3d_lds.h: conv3d_wgrad_assign deals (chunk, kd) and the remaining tiles to the workgroups of
  conv3d_wgrad_lds_kernel.  Through as_conv3d_wgrad_lds_assignment (the same function, run on the host) for many
  (ntiles, nchunks) — multiples of 8 or not, tiles remaining or not: every tile is accumulated by exactly three workgroups,
  one per kd; padding blocks own nothing.  (Round 4 numbered the extra tiles over the padded grid: with nchunks % 8 != 0 and
  tiles remaining some were never accumulated.)"""
  import ctypes
  from adaptive_stereo import _native as nat
  lib = nat.load()
  cases = [(576, 168), (144, 144), (1632, 168), (170, 165), (100, 13), (37, 9), (64, 64), (65, 64), (1000, 167), (23, 1), (17, 17),
           (200, 171), (9, 8), (15, 8), (16, 9)]
  for ntiles, nchunks in cases:
    per_xcd = (nchunks + 7) // 8
    seen = {}
    working = 0
    for block in range(8 * per_xcd * 3):
      c, kd, ex = ctypes.c_int(-9), ctypes.c_int(-9), ctypes.c_int(-9)
      rc = lib.as_conv3d_wgrad_lds_assignment(ntiles, nchunks, block, ctypes.byref(c), ctypes.byref(kd), ctypes.byref(ex))
      assert rc in (0, 1)
      if rc == 0:
        continue
      working += 1
      assert 0 <= c.value < nchunks and 0 <= kd.value < 3
      tiles = [c.value + k * nchunks for k in range(ntiles // nchunks)] + ([ex.value] if ex.value >= 0 else [])
      for t in tiles:
        assert 0 <= t < ntiles, (ntiles, nchunks, block, t)
        seen.setdefault(t, []).append(kd.value)
    assert working == 3 * nchunks, (ntiles, nchunks, working)
    assert sorted(seen) == list(range(ntiles)), (ntiles, nchunks, "tiles never accumulated: %s" % sorted(set(range(ntiles)) - set(seen))[:8])
    assert all(sorted(v) == [0, 1, 2] for v in seen.values()), (ntiles, nchunks)
