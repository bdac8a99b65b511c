"""bench.py on one GPU, as the driver runs it: a plain run prints the headline line and nothing else; --full adds every other
measurement to the same line."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

from conftest import REPO

HEADLINE = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"}
FULL_ONLY = {"eager_ms_per_step", "fwd_pairs_per_s", "fwd_ms_per_step", "roofline", "sustained", "batch16", "sceneflow_fwd",
             "online_batch1", "dp_path_overhead_ms", "cpu_baseline"}


def _bench(args, tmp_path, tag):
  out_path, err_path = tmp_path / ("bench_%s.out" % tag), tmp_path / ("bench_%s.err" % tag)
  with open(out_path, "w") as fo, open(err_path, "w") as fe:
    rc = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1"] + args, stdout=fo, stderr=fe,
                        cwd=str(tmp_path), timeout=600).returncode
  err = open(err_path).read()
  assert rc == 0, err[-3000:]
  lines = [l for l in open(out_path).read().splitlines() if l.strip()]
  assert len(lines) == 1, "bench.py must print ONE line on stdout, got %d: %r" % (len(lines), lines[:3])
  return json.loads(lines[0]), err


def test_plain_run_prints_the_headline_alone(tmp_path):
  """The default workload: warm-up, the timed steps, the dump, the line; none of the --full measurements."""
  dump = tmp_path / "dump"
  line, err = _bench(["--steps", "3", "--warmup", "2", "--dump-outputs", str(dump)], tmp_path, "plain")
  assert HEADLINE <= set(line) and not FULL_ONLY & set(line), sorted(line)
  assert line["steps"] == 3 and line["warmup"] == 2 and line["higher_is_better"] is True and line["dtype"] == "f32"
  assert line["unit"] == "stereo pairs/s" and line["metric"].startswith("stereo pairs/sec")
  assert line["value"] > 0 and abs(line["value"] - 4 * 3 / (3 * line["ms_per_step"] * 1e-3)) <= 0.01 * line["value"]
  assert line["launch_mode"] == "hipGraph replay of the captured step (1 graph)"
  assert "timed forward" not in err and "cpu baseline" not in err
  assert (dump / "loss.npy").exists() and (dump / "outputs.pred_disp_l.0.npy").exists()


def test_full_run_carries_every_leg(tmp_path):
  """--full at a small size (its legs at their own sizes): the forward-only rate, the roofline and every side leg."""
  line, err = _bench(["--steps", "2", "--warmup", "1", "--batch", "2", "--height", "96", "--width", "256", "--full"], tmp_path,
                     "full")
  assert HEADLINE <= set(line) and FULL_ONLY <= set(line), sorted(FULL_ONLY - set(line))
  assert line["value"] > 0 and line["fwd_pairs_per_s"] > 0 and line["eager_ms_per_step"] > 0
  assert line["roofline"] is not None and line["roofline"]["achieved"] > 0
  assert line["sustained"]["steps"] >= 50 and line["batch16"]["pairs_per_s"] > 0 and line["sceneflow_fwd"]["pairs_per_s"] > 0
  assert line["online_batch1"]["pairs_per_s"] > 0
  assert line["dp_path_overhead_ms"]["value"] is not None, line["dp_path_overhead_ms"]
  assert line["cpu_baseline"]["value"] > 0 and "parity" in line["cpu_baseline"]
  assert "side_legs_error" not in line
