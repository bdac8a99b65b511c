"""The reference's train.py: supervised StereoNet training (train.train, train.py:140-243) and the part other scripts import
(adapt.py:13, evaluate_model.py:10): TrainOptions, process_batch, evaluate, log_scalars, log_images, save_models —
SURVEY.md §8b / §8f-3.

``train`` is the reference's loop: seed 123, opt.json, the two StereoDatasets with scales [s, s + k] (random crop and optional
flip for training), the evaluate / log_scalars / log_images cadence, a checkpoint per ``save_freq`` epochs from epoch 1 on and
one at the end, StepLR(scheduler_step_size, 0.5).  The step itself is adaptive_stereo.training.SupervisedTrainer: the two-scale
Khamis loss as one fused node, clip + Adam over flat arenas, the whole step one captured hipGraph from the second full batch on
(the schedule reaches it through a device scalar; a last, smaller batch of an epoch runs eagerly).  ``--load_weights_folder``
and ``--load_adam`` resume from a checkpoint folder (with ``--load_adam`` at the checkpoint's learning rate).  tensorboardX
and gitpython are optional: without a writer only the console summary is printed, and the commit hash in opt.json comes from
``git rev-parse HEAD`` or is "unknown".

``evaluate`` keeps the reference's definition of the metrics (train.py:74-126: per-batch EPE over gt>0,
D1-all at 2/3/4/5 px, FCS mean; then the mean over batches) but computes each batch's reductions in one
fused kernel (as_eval_metrics) and reads nothing back until the loop has finished.
"""
import argparse
import json
import os
import time

import torch

from adaptive_stereo import _native as nat
from adaptive_stereo.collect import stereo_forward
from adaptive_stereo.utils.feature_contrast import feature_contrast_mean


class TrainOptions(object):
  """Same flags and defaults as the reference (train.py:246-301)."""

  def __init__(self):
    p = argparse.ArgumentParser(description="Options for StereoNet adaptation on MI355X")
    p.add_argument("--height", type=int, default=320)
    p.add_argument("--width", type=int, default=960)
    p.add_argument("--model_name", type=str)
    p.add_argument("--stereonet_input_scale", default=0, type=int)
    p.add_argument("--stereonet_k", type=int, default=3, choices=[3, 4])
    p.add_argument("--dataset_path", type=str)
    p.add_argument("--dataset_name", type=str, default="SceneFlowDriving")
    p.add_argument("--split", type=str)
    p.add_argument("--batch_size", type=int, default=2)
    p.add_argument("--do_hflip", action="store_true", default=False)
    p.add_argument("--no_shuffle", action="store_true", default=False)
    p.add_argument("--use_grayscale", action="store_true")
    p.add_argument("--log_dir", type=str, default="/home/milo/training_logs")
    p.add_argument("--load_weights_folder", default=None, type=str)
    p.add_argument("--load_adam", action="store_true", default=False)
    p.add_argument("--scheduler_step_size", default=5, type=int)
    p.add_argument("--num_workers", type=int, default=4)
    p.add_argument("--num_epochs", type=int, default=100)
    p.add_argument("--log_frequency", type=int, default=250)
    p.add_argument("--save_freq", type=int, default=1)
    p.add_argument("--fast_eval", action="store_true", default=False)
    p.add_argument("--learning_rate", default=1e-5, type=float)
    p.add_argument("--clip_grad_norm", action="store_true", default=False)
    p.add_argument("--leftright_consistency", action="store_true", default=False)
    p.add_argument("--smoothness_weight", type=float, default=1e-3)
    p.add_argument("--consistency_weight", type=float, default=1e-3)
    p.add_argument("--num_steps", type=int, default=-1)
    p.add_argument("--ovs_buffer_size", type=int, default=10)
    p.add_argument("--skip_initial_eval", action="store_true")
    p.add_argument("--ovs_validate_hz", type=int, default=100)
    p.add_argument("--adapt_mode", choices=["NONSTOP", "VS", "ER", "VS+ER", "NONE"])
    p.add_argument("--val_improve_retries", type=int, default=1)
    p.add_argument("--eval_hz", type=int, default=1000)
    p.add_argument("--er_loss_weight", type=float, default=0.05)
    p.add_argument("--train_dataset_path", type=str)
    p.add_argument("--train_dataset_name", type=str)
    p.add_argument("--train_split", type=str)
    p.add_argument("--ood_threshold", type=float, default=15.0)
    p.add_argument("--fcs_ema_weight", type=float, default=0.999)
    p.add_argument("--no_capture", action="store_true", default=False,
                   help="adapt.py: the host-side adaptation loop instead of the captured, device-gated one")
    p.add_argument("--proxy_loss_weight", type=float, default=0.0,
                   help="adapt.py: weight of the Khamis loss against semi-global-matching proxy labels (0: no matcher is built)")
    p.add_argument("--proxy_only", action="store_true", default=False,
                   help="adapt.py: back-propagate the proxy term alone (the photometric loss is still computed and reported)")
    p.add_argument("--proxy_paths", type=int, default=8, choices=[4, 8], help="adapt.py: aggregation paths of the matcher")
    p.add_argument("--proxy_uniqueness", type=int, default=5, help="adapt.py: the matcher's uniqueness margin in per cent")
    p.add_argument("--proxy_max_size", type=int, default=200, help="adapt.py: largest speckle the label filter removes, in pixels")
    p.add_argument("--ovs_metric", choices=["photometric", "proxy_epe"], default="photometric",
                   help="adapt.py: what the online validation set is scored by (proxy_epe needs --proxy_loss_weight > 0)")
    self.parser = p

  def parse(self, args=None):
    self.options = self.parser.parse_args(args)
    return self.options


def process_batch(feature_net, stereo_net, left, right, opt, output_cost_volume=False):
  """Reference train.py:19-22 (collect.stereo_forward)."""
  return stereo_forward(feature_net, stereo_net, left, right, output_cost_volume=output_cost_volume)


def disparity_metrics(pred_disp, gt_disp):
  """-> device tensor [EPE, D1_all_2px, D1_all_3px, D1_all_4px, D1_all_5px] for one batch (no host sync)."""
  nat.require_gpu(pred_disp, gt_disp)
  pred, gt = nat.f32c(pred_disp), nat.f32c(gt_disp)
  n = pred.numel()
  out6 = torch.empty(6, dtype=torch.float32, device=pred.device)
  ws = torch.empty(nat.load().as_eval_metrics_workspace(n), dtype=torch.float32, device=pred.device)
  nat.call("as_eval_metrics", nat.ptr(pred), nat.ptr(gt), n, nat.ptr(out6), nat.ptr(ws), nat.stream())
  return torch.cat([out6[0:1], out6[2:6]]) / out6[1]


def evaluate(feature_net, stereo_net, val_loader, opt):
  """Metrics dict {"EPE", "FCS", "D1_all_{2,3,4,5}px"} exactly as train.py:74-126 defines them."""
  was_training = feature_net.training
  feature_net.eval(); stereo_net.eval()
  n_eval = len(val_loader) // 10 if getattr(opt, "fast_eval", False) else len(val_loader)
  if getattr(opt, "num_steps", -1) > 0:
    n_eval = min(opt.num_steps // val_loader.batch_size, len(val_loader))
  s, k = opt.stereonet_input_scale, opt.stereonet_k
  rows, fcs = [], []
  with torch.no_grad():
    for i, inputs in enumerate(val_loader):
      if i >= n_eval:
        break
      left = inputs["color_l/{}".format(s)].cuda()
      right = inputs["color_r/{}".format(s)].cuda()
      gt = inputs["gt_disp_l/{}".format(s)].cuda()
      outputs = process_batch(feature_net, stereo_net, left, right, opt, output_cost_volume=True)
      rows.append(disparity_metrics(outputs["pred_disp_l/{}".format(s)], gt))
      fcs.append(feature_contrast_mean(outputs["cost_volume_l/{}".format(s + k)]).mean())
    m = torch.stack(rows).mean(dim=0).cpu() if rows else torch.zeros(5)
    f = float(torch.stack(fcs).mean()) if fcs else 0.0
  feature_net.train(was_training); stereo_net.train(was_training)
  return {"EPE": float(m[0]), "FCS": f, "D1_all_2px": float(m[1]), "D1_all_3px": float(m[2]),
          "D1_all_4px": float(m[3]), "D1_all_5px": float(m[4])}


def log_scalars(writer, metrics, losses, examples_per_sec, epoch, step):
  """Console summary (+ scalars to `writer` when one is given; tensorboardX is not a dependency here)."""
  if writer is not None:
    for name in losses:
      writer.add_scalar(name, float(losses[name]), step)
    for name in metrics:
      writer.add_scalar(name, float(metrics[name]), step)
    writer.add_scalar("examples_per_sec", examples_per_sec, step)
  print("\n{}|{} examples/sec={:.3f}".format(epoch, step, examples_per_sec))
  if metrics:
    print("METRICS // " + " | ".join("{}={:.3f}".format(k, float(v)) for k, v in sorted(metrics.items())))
  if losses:
    print("LOSS    // " + " | ".join("{}={:.3f}".format(k, float(v)) for k, v in losses.items()))


def log_images(writer, inputs, outputs, step, skip_prefixes=("cost_volume",), disp_cmap=None):
  """disp_cmap None: every image is logged as it is.  A colour map (a packaged name or a Colormap object): entries whose name
  contains "disp" are colour-mapped on the device over their own range first, as the reference's train.py:60-71 does on the
  host with magma; [3,H,W] fp32."""
  if writer is None:
    return
  for io in (inputs, outputs):
    for name in io:
      if any(p in name for p in skip_prefixes):
        continue
      image = io[name][0].detach().float()
      if disp_cmap is not None and "disp" in name:
        from adaptive_stereo.utils.visualization import colormap
        image = colormap(image.reshape((1, 1) + tuple(image.shape[-2:])), cmap=disp_cmap, out="f32")[0]
      writer.add_image(name, image.cpu(), step)


def save_models(feature_net, stereo_net, optimizer, log_path, epoch):
  """<log_path>/models/weights_<epoch>/{feature_net,stereo_net,adam}.pth (train.py:129-137).  The state
  dicts are cloned to the CPU first: parameters here are views into a flat arena."""
  folder = os.path.join(log_path, "models", "weights_{}".format(epoch))
  os.makedirs(folder, exist_ok=True)
  for name, net in (("feature_net", feature_net), ("stereo_net", stereo_net)):
    torch.save({k: v.detach().cpu().clone() for k, v in net.state_dict().items()}, os.path.join(folder, name + ".pth"))
  if optimizer is not None:
    torch.save(optimizer.state_dict(), os.path.join(folder, "adam.pth"))
  return folder


def load_models(feature_net, stereo_net, folder, strict=True):
  """adapt.py:203-206."""
  feature_net.load_state_dict(torch.load(os.path.join(folder, "feature_net.pth"), map_location="cpu"), strict=strict)
  stereo_net.load_state_dict(torch.load(os.path.join(folder, "stereo_net.pth"), map_location="cpu"), strict=strict)


def _commit_hash():
  import subprocess
  try:
    r = subprocess.run(["git", "rev-parse", "HEAD"], cwd=os.path.dirname(os.path.abspath(__file__)), capture_output=True,
                       text=True, timeout=10)
    sha = r.stdout.strip()
    return sha if r.returncode == 0 and sha else "unknown"
  except (OSError, subprocess.SubprocessError):
    return "unknown"


def _summary_writer(path):
  try:
    from tensorboardX import SummaryWriter
  except ImportError:
    print("tensorboardX is not installed: console summaries only")
    return None
  return SummaryWriter(path)


def train(opt, train_dataset=None, val_dataset=None, writer=None):
  """Reference train.py:140-243.  ``train_dataset`` / ``val_dataset`` (map-style datasets of the StereoDataset sample
  dictionary) and ``writer`` (add_scalar / add_image) replace what the options would build.  Returns the SupervisedTrainer."""
  from torch.utils.data import DataLoader
  from adaptive_stereo.models.stereo_net import StereoNet, FeatureExtractorNetwork
  from adaptive_stereo.training import SupervisedTrainer

  torch.manual_seed(123)
  log_path = os.path.join(opt.log_dir, opt.model_name)
  os.makedirs(log_path, exist_ok=True)
  opt.commit_hash = _commit_hash()
  with open(os.path.join(log_path, "opt.json"), "w") as f:
    opt_readable = json.dumps(opt.__dict__, sort_keys=True, indent=2)
    print("TRAINING OPTIONS:\n" + opt_readable)
    f.write(opt_readable + "\n")

  s, k = opt.stereonet_input_scale, opt.stereonet_k
  feature_net = FeatureExtractorNetwork(k).cuda()
  stereo_net = StereoNet(k, 1, s).cuda()
  if opt.load_weights_folder is not None:
    print("Loading models from: ", opt.load_weights_folder)
    load_models(feature_net, stereo_net, opt.load_weights_folder, strict=True)
  trainer = SupervisedTrainer(feature_net, stereo_net, lr=opt.learning_rate, clip_grad_norm=opt.clip_grad_norm)
  optimizer = trainer.optimizer
  if opt.load_adam:
    if opt.load_weights_folder is None:
      raise ValueError("--load_adam needs --load_weights_folder")
    optimizer.load_state_dict(torch.load(os.path.join(opt.load_weights_folder, "adam.pth"), map_location="cpu"))
  base_lr = optimizer.lr

  loss_scales = [s, s + k]
  if train_dataset is None:
    from adaptive_stereo.datasets.stereo_dataset import StereoDataset
    train_dataset = StereoDataset(opt.dataset_path, opt.dataset_name, opt.split, opt.height, opt.width, "train",
                                  scales=loss_scales, do_hflip=opt.do_hflip, random_crop=True, load_disp_left=True,
                                  load_disp_right=True)
  if val_dataset is None:
    from adaptive_stereo.datasets.stereo_dataset import StereoDataset
    val_dataset = StereoDataset(opt.dataset_path, opt.dataset_name, opt.split, opt.height, opt.width, "val",
                                scales=loss_scales, do_hflip=False, random_crop=False, load_disp_left=True,
                                load_disp_right=False)
  pin = opt.num_workers > 0
  train_loader = DataLoader(train_dataset, opt.batch_size, not opt.no_shuffle, num_workers=opt.num_workers, pin_memory=pin,
                            drop_last=False)
  val_loader = DataLoader(val_dataset, opt.batch_size, False, num_workers=opt.num_workers, pin_memory=pin, drop_last=False)
  print("DATASET SIZES:\n  TRAIN={} VAL={}".format(len(train_dataset), len(val_dataset)))
  if writer is None:
    writer = _summary_writer(os.path.join(log_path, "val"))

  epoch, step = 0, 0
  for epoch in range(opt.num_epochs):
    feature_net.train(); stereo_net.train()
    for bi, inputs in enumerate(train_loader):
      t0 = time.time()
      inputs = {key: value.cuda(non_blocking=True) for key, value in inputs.items()}
      left, right = inputs["color_l/{}".format(s)], inputs["color_r/{}".format(s)]
      gt = inputs["gt_disp_l/{}".format(s)]
      result = trainer.step(left, right, gt)
      outputs = result["outputs"]
      losses = {name: value for name, value in result.items() if name != "outputs"}
      if trainer.graph_count() == 0 and left.shape[0] == opt.batch_size:
        trainer.capture(left, right, gt)            # after the first full batch; leaves the training state as it is
      early_phase = (step % opt.log_frequency) == 0 and step < 2000
      late_phase = (step % 2000) == 0 or (bi == 0)          # at the start of each epoch
      if early_phase or late_phase:
        torch.cuda.synchronize()
        elapsed_this_batch = time.time() - t0
        metrics = evaluate(feature_net, stereo_net, val_loader, opt)
        log_scalars(writer, metrics, losses, opt.batch_size / elapsed_this_batch, epoch, step)
        log_images(writer, inputs, outputs, step)
      step += 1
    if epoch >= 1 and (epoch % opt.save_freq) == 0:
      save_models(feature_net, stereo_net, optimizer, log_path, epoch)
    trainer.set_lr(base_lr * 0.5 ** ((epoch + 1) // opt.scheduler_step_size))        # StepLR(scheduler_step_size, 0.5).step()
  save_models(feature_net, stereo_net, optimizer, log_path, epoch)         # a final save after training
  return trainer


if __name__ == "__main__":
  train(TrainOptions().parse())
  print("Done with training!")
