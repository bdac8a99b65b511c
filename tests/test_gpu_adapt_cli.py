"""adapt.adapt() end to end on injected list datasets: trials.csv, the checkpoints, the metrics, a second trial appended, and
the captured loop against --no_capture."""
import csv
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from adaptive_stereo.models.stereo_net import StereoNet, FeatureExtractorNetwork
from adaptive_stereo.utils import synthetic as syn

K, H, W = 3, 64, 96


class ListDataset(torch.utils.data.Dataset):
  def __init__(self, samples):
    self.samples = samples

  def __len__(self):
    return len(self.samples)

  def __getitem__(self, i):
    return self.samples[i]


def _samples(seed, n):
  left, right = syn.stereo_pair(n, H, W, seed=seed, disparities=(3.0, 6.0, 4.0))
  gt = torch.rand(n, 1, H, W, generator=torch.Generator().manual_seed(seed)) * 20 + 1
  gt[:, :, ::3, ::4] = 0.0
  return [{"color_l/0": left[i], "color_r/0": right[i], "gt_disp_l/0": gt[i]} for i in range(n)]


def _weights_folder(path):
  import train as train_module
  fnet, snet = FeatureExtractorNetwork(K), StereoNet(K, 1, 0)
  fnet.load_state_dict(syn.synthetic_state_dict(fnet.state_dict(), seed=123))
  snet.load_state_dict(syn.synthetic_state_dict(snet.state_dict(), seed=123, logit_gain=5.0))
  return train_module.save_models(fnet, snet, None, str(path), 0)


def _options(tmp_path, folder, *extra):
  import train as train_module
  return train_module.TrainOptions().parse([
      "--height", str(H), "--width", str(W), "--model_name", "run", "--log_dir", str(tmp_path), "--batch_size", "1",
      "--stereonet_k", str(K), "--num_epochs", "5", "--num_workers", "0", "--learning_rate", "1e-3", "--clip_grad_norm",
      "--adapt_mode", "VS+ER", "--num_steps", "6", "--eval_hz", "3", "--ovs_validate_hz", "4", "--log_frequency", "2",
      "--ood_threshold", "1e30", "--fcs_ema_weight", "0.5", "--load_weights_folder", folder] + list(extra))


def test_adapt_end_to_end(tmp_path):
  """Three pairs per epoch, every one novel (threshold 1e30), a reservoir of ten: steps 0-2 fill the reservoir without an
  update, steps 3-5 offer the same batch indices again, are refused and update — whatever the FCS is.  The buffer never fills,
  so no random number is drawn and --no_capture must end at the same parameters."""
  import adapt as adapt_module
  import train as train_module
  from torch.utils.data import DataLoader
  stream, adapt_val, train_val = _samples(5, 3), _samples(6, 2), _samples(7, 2)
  folder = _weights_folder(tmp_path / "pretrained")

  class Writer(object):
    def __init__(self):
      self.scalars = []

    def add_scalar(self, name, value, step):
      self.scalars.append((name, step))

    def add_image(self, name, image, step):
      pass

  writer = Writer()
  opt = _options(tmp_path, folder)
  loop = adapt_module.adapt(opt, ListDataset(stream), ListDataset(adapt_val), ListDataset(train_val), writer=writer)
  assert loop.captured and loop.graph_count() == 1 and loop.step == 6
  assert loop.gradient_updates == 3 == loop.adapter.optimizer.step_count
  assert loop.state_machine.ovs.counters() == (3, 6, 3, 3)
  log_path = os.path.join(str(tmp_path), "run")
  saved = json.load(open(os.path.join(log_path, "opt.json")))
  assert saved["adapt_mode"] == "VS+ER" and saved["no_capture"] is False and "commit_hash" in saved
  assert ("EPE", 2) in writer.scalars and ("Replay/total_loss", 4) in writer.scalars and ("GRADIENT_UPDATES", 6) in writer.scalars

  rows = list(csv.reader(open(os.path.join(log_path, "trials.csv"), newline="")))
  assert tuple(rows[0]) == adapt_module.TRIALS_COLUMNS
  assert rows[0][:2] == ["trial", "step"] and rows[0][-1] == "GRADIENT_UPDATES" and "EPE_ADAPT" in rows[0] and "D1_all_3px_TRAIN" in rows[0]
  table = adapt_module.read_trials(os.path.join(log_path, "trials.csv"))
  assert [(r["trial"], r["step"], r["GRADIENT_UPDATES"]) for r in table] == [("0", "-1", ""), ("0", "3", "0"), ("0", "6", "3")]

  # checkpoints at steps 3 and 6, adam.pth at the number of updates really made (none before step 3, three by step 6)
  assert sorted(os.listdir(os.path.join(log_path, "models"))) == ["weights_3", "weights_6"]
  adam3 = torch.load(os.path.join(log_path, "models", "weights_3", "adam.pth"), map_location="cpu")
  adam6 = torch.load(os.path.join(log_path, "models", "weights_6", "adam.pth"), map_location="cpu")
  assert len(adam3["state"]) == 0
  assert len(adam6["state"]) > 0 and {float(st["step"]) for st in adam6["state"].values()} == {3.0}

  # the last row's metrics are evaluate()'s on the final weights
  fnet, snet = loop.adapter.feature_net, loop.adapter.stereo_net
  for suffix, samples in (("_ADAPT", adapt_val), ("_TRAIN", train_val)):
    m = train_module.evaluate(fnet, snet, DataLoader(ListDataset(samples), 6, False), opt)
    for name in adapt_module.METRIC_NAMES:
      assert float(table[-1][name + suffix]) == m[name], (name, suffix)
  sd = torch.load(os.path.join(log_path, "models", "weights_6", "stereo_net.pth"), map_location="cpu")
  for key, t in snet.state_dict().items():
    assert torch.equal(sd[key], t.detach().cpu()), key
  first = float(table[0]["EPE_ADAPT"])
  assert first > 0 and first != float(table[-1]["EPE_ADAPT"])

  # a second trial in the same folder, on the host-side loop: appended as trial 1, the same final parameters bit for bit
  opt2 = _options(tmp_path, folder, "--no_capture")
  loop2 = adapt_module.adapt(opt2, ListDataset(stream), ListDataset(adapt_val), ListDataset(train_val), writer=writer)
  assert not loop2.captured and loop2.gradient_updates == 3
  table2 = adapt_module.read_trials(os.path.join(log_path, "trials.csv"))
  assert [(r["trial"], r["step"]) for r in table2] == [("0", "-1"), ("0", "3"), ("0", "6"), ("1", "-1"), ("1", "3"), ("1", "6")]
  assert table2[:3] == table
  assert torch.equal(loop.adapter.arena.params, loop2.adapter.arena.params)
  assert torch.equal(loop.adapter.optimizer.exp_avg_sq, loop2.adapter.optimizer.exp_avg_sq)
  for col in adapt_module.TRIALS_COLUMNS[2:]:
    assert table2[5][col] == table2[2][col], col


def test_adapt_refuses_leftright_consistency(tmp_path):
  import adapt as adapt_module
  opt = _options(tmp_path, "unused", "--leftright_consistency")
  with pytest.raises(NotImplementedError, match="SURVEY"):
    adapt_module.adapt(opt, ListDataset([]), ListDataset([]), ListDataset([]))
