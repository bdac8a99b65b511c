"""The reference's adapt.py: online adaptation of a trained StereoNet to a new domain (adapt.adapt, adapt.py:187-443) in the
modes NONSTOP, VS, ER, VS+ER and NONE — SURVEY.md §8f-2.

``adapt`` is the reference's loop: opt.json, the three StereoDatasets with scales [s, s + k] (the adaptation stream, its
validation split, the training domain's validation split), the pre-adaptation evaluation (row ``step = -1`` of trials.csv), one
pair of the training domain per step for experience replay (``train_val_dataset[step % len]``), the per-step EPE log, an
evaluation of both validation sets plus a checkpoint plus a trials.csv row every ``--eval_hz`` steps, the stop at ``--num_steps``.
A later run in the same folder appends the next trial.  The step itself is adaptive_stereo.control.AdaptationLoop over an
OnlineAdapter; by default the captured one (every IN_PROGRESS step one hipGraph replay, the gate decided on the device),
``--no_capture`` runs the host-side loop.  tensorboardX is optional, as in train.py.

``--leftright_consistency`` raises NotImplementedError: the reference's path is dead code (adapt.py:319 reads the
misspelt ``opt.stereonet_intput_scale`` and monodepth_leftright_loss overwrites its own ``outputs`` argument), so there is no
behaviour to reproduce.
"""
import csv
import json
import os
import time

import torch

from train import (TrainOptions, evaluate, log_scalars, log_images, save_models, load_models, _commit_hash,
                   _summary_writer)

METRIC_NAMES = ("EPE", "FCS", "D1_all_2px", "D1_all_3px", "D1_all_4px", "D1_all_5px")
TRIALS_COLUMNS = ("trial", "step") + tuple(m + "_ADAPT" for m in METRIC_NAMES) + tuple(m + "_TRAIN" for m in METRIC_NAMES) + \
    ("GRADIENT_UPDATES",)


LEFTRIGHT_LOSS_MESSAGE = ("--leftright_consistency: the reference's left-right path cannot run (adapt.py:319 reads the "
                          "misspelt opt.stereonet_intput_scale, and monodepth_leftright_loss overwrites its own outputs "
                          "argument: SURVEY.md 0.8), so there is no behaviour to reproduce")


def predict_disparity_leftright(feature_net, stereo_net, left, right, adapt_state, opt):
  """Reference adapt.py:40-62: the left AND the right disparity maps of a batch from one pass over the mirrored batches, keys
  ``..._l/..`` and ``..._r/..``.  The inference half runs (adaptive_stereo.consistency) for State.VALIDATION and State.DONE, the two
  states in which the reference computes no gradients and has its networks in eval mode; State.IN_PROGRESS would feed the
  reference's dead left-right loss and raises as the flag does; anything else is not a state."""
  from adaptive_stereo.consistency import predict_disparity_leftright as both_views
  from adaptive_stereo.control import State
  if adapt_state == State.IN_PROGRESS:
    raise NotImplementedError(LEFTRIGHT_LOSS_MESSAGE)
  if adapt_state not in (State.VALIDATION, State.DONE):
    raise ValueError("predict_disparity_leftright: adapt_state %r (State.VALIDATION or State.DONE)" % (adapt_state,))
  return both_views(feature_net, stereo_net, left, right, output_cost_volume=True)


def read_trials(path):
  """Rows of a trials.csv as dictionaries of strings ([] when the file does not exist)."""
  if not os.path.exists(path):
    return []
  with open(path, newline="") as f:
    return list(csv.DictReader(f))


def append_trial_row(path, trial, step, metrics_adapt, metrics_train, gradient_updates=None):
  """One row of the reference's table (adapt.py:175-184): the columns of TRIALS_COLUMNS; GRADIENT_UPDATES is empty in the row of
  the initial evaluation, as pandas leaves it."""
  row = {"trial": trial, "step": step, "GRADIENT_UPDATES": "" if gradient_updates is None else gradient_updates}
  row.update({k + "_ADAPT": v for k, v in metrics_adapt.items()})
  row.update({k + "_TRAIN": v for k, v in metrics_train.items()})
  new = not os.path.exists(path)
  with open(path, "a", newline="") as f:
    w = csv.DictWriter(f, fieldnames=TRIALS_COLUMNS, extrasaction="raise")
    if new:
      w.writeheader()
    w.writerow({k: repr(v) if isinstance(v, float) else v for k, v in row.items()})


def proxy_labeler_from_options(opt, stereo_net):
  """The sgm.ProxyLabeler that --proxy_loss_weight > 0 asks for (None otherwise): at the resolution and batch size the step
  runs at, over the network's own disparity range, which the matcher takes up to 256."""
  if getattr(opt, "proxy_loss_weight", 0.0) <= 0.0:
    if getattr(opt, "proxy_only", False) or getattr(opt, "ovs_metric", "photometric") == "proxy_epe":
      raise ValueError("--proxy_only and --ovs_metric proxy_epe need --proxy_loss_weight above 0")
    return None
  from adaptive_stereo.sgm import ProxyLabeler
  if stereo_net.maxdisp > 256:
    raise ValueError("--proxy_loss_weight: the network's maxdisp %d is beyond the matcher's 256" % stereo_net.maxdisp)
  s = opt.stereonet_input_scale
  return ProxyLabeler(opt.height >> s, opt.width >> s, batch=opt.batch_size, maxdisp=stereo_net.maxdisp, paths=opt.proxy_paths,
                      uniqueness=opt.proxy_uniqueness, max_size=opt.proxy_max_size)


def adapt(opt, adapt_dataset=None, adapt_val_dataset=None, train_val_dataset=None, writer=None):
  """Reference adapt.py:187-443.  The datasets (map-style, of the StereoDataset sample dictionary) and ``writer`` (add_scalar /
  add_image) replace what the options would build.  Returns the AdaptationLoop."""
  from torch.utils.data import DataLoader
  from adaptive_stereo.adaptation import OnlineAdapter
  from adaptive_stereo.control import AdaptationLoop
  from adaptive_stereo.models.stereo_net import StereoNet, FeatureExtractorNetwork

  if opt.leftright_consistency:
    raise NotImplementedError(LEFTRIGHT_LOSS_MESSAGE)
  if opt.adapt_mode is None:
    raise ValueError("--adapt_mode is required (NONSTOP, VS, ER, VS+ER or NONE)")
  torch.manual_seed(123)
  log_path = os.path.join(opt.log_dir, opt.model_name)
  os.makedirs(log_path, exist_ok=True)
  opt.commit_hash = _commit_hash()
  with open(os.path.join(log_path, "opt.json"), "w") as f:
    opt_readable = json.dumps(opt.__dict__, sort_keys=True, indent=4)
    print("ADAPTATION OPTIONS:\n" + opt_readable)
    f.write(opt_readable + "\n")

  s, k = opt.stereonet_input_scale, opt.stereonet_k
  feature_net = FeatureExtractorNetwork(k).cuda()
  stereo_net = StereoNet(k, 1, s).cuda()
  if opt.load_weights_folder is not None:
    print("Loading models from: ", opt.load_weights_folder)
    load_models(feature_net, stereo_net, opt.load_weights_folder, strict=True)

  image_scales = [s, s + k]
  if adapt_dataset is None or adapt_val_dataset is None or train_val_dataset is None:
    from adaptive_stereo.datasets.stereo_dataset import StereoDataset
  if adapt_dataset is None:
    adapt_dataset = StereoDataset(opt.dataset_path, opt.dataset_name, opt.split, opt.height, opt.width, "train",
                                  scales=image_scales, do_hflip=False, random_crop=False, load_disp_left=True,
                                  load_disp_right=True)
  if adapt_val_dataset is None:
    adapt_val_dataset = StereoDataset(opt.dataset_path, opt.dataset_name, opt.split, opt.height, opt.width, "val",
                                      scales=image_scales, do_hflip=False, random_crop=False, load_disp_left=True,
                                      load_disp_right=False)
  er_mode = opt.adapt_mode in ("ER", "VS+ER")
  if train_val_dataset is None:
    train_val_dataset = StereoDataset(opt.train_dataset_path, opt.train_dataset_name, opt.train_split, opt.height, opt.width,
                                      "val", scales=image_scales, do_hflip=False, random_crop=False, load_disp_left=True,
                                      load_disp_right=False)
  pin = opt.num_workers > 0
  adapt_loader = DataLoader(adapt_dataset, opt.batch_size, False, num_workers=opt.num_workers, pin_memory=pin, drop_last=False)
  adapt_val_loader = DataLoader(adapt_val_dataset, 6, False, num_workers=opt.num_workers, pin_memory=pin, drop_last=False)
  train_val_loader = DataLoader(train_val_dataset, 6, False, num_workers=opt.num_workers, pin_memory=pin, drop_last=False)
  print("DATASET SIZES:\n  TRAIN={} VAL={}".format(len(adapt_dataset), len(adapt_val_dataset)))
  adapt_writer, train_writer = writer, writer
  if writer is None:
    adapt_writer = _summary_writer(os.path.join(log_path, "adapt"))
    train_writer = _summary_writer(os.path.join(log_path, "train")) if adapt_writer is not None else None

  labeler = proxy_labeler_from_options(opt, stereo_net)
  adapter = OnlineAdapter(feature_net, stereo_net, opt.height >> s, opt.width >> s, lr=opt.learning_rate,
                          clip_grad_norm=opt.clip_grad_norm, smoothness_weight=opt.smoothness_weight,
                          fcs_ema_weight=opt.fcs_ema_weight, proxy_labeler=labeler,
                          proxy_loss_weight=getattr(opt, "proxy_loss_weight", 0.0), proxy_only=getattr(opt, "proxy_only", False))
  loop = AdaptationLoop(adapter, mode=opt.adapt_mode, ovs_buffer_size=opt.ovs_buffer_size, ovs_validate_hz=opt.ovs_validate_hz,
                        val_improve_retries=opt.val_improve_retries, ood_threshold=opt.ood_threshold,
                        er_loss_weight=opt.er_loss_weight, captured=not getattr(opt, "no_capture", False),
                        ovs_metric=getattr(opt, "ovs_metric", "photometric"))

  trials_path = os.path.join(log_path, "trials.csv")
  previous = read_trials(trials_path)
  trial_index = max(int(r["trial"]) for r in previous) + 1 if previous else 0
  print("\nNOTE: {} trials.csv, running trial #{}".format("Found existing" if previous else "No existing", trial_index))

  if not opt.skip_initial_eval:
    print("========================= PRE-ADAPTATION EVALUATION ============================")
    metrics_adapt = evaluate(feature_net, stereo_net, adapt_val_loader, opt)
    log_scalars(adapt_writer, metrics_adapt, {}, 0, 0, 0)
    metrics_train = evaluate(feature_net, stereo_net, train_val_loader, opt)
    log_scalars(train_writer, metrics_train, {}, 0, 0, 0)
    append_trial_row(trials_path, trial_index, -1, metrics_adapt, metrics_train)
  else:
    print("----------------- WARNING: Skipped pre-adaptation evaluation -------------------")

  left_key, right_key, gt_key = "color_l/{}".format(s), "color_r/{}".format(s), "gt_disp_l/{}".format(s)
  epoch, step = 0, 0
  for epoch in range(opt.num_epochs):
    if opt.num_steps > 0 and step >= opt.num_steps:
      break
    t0_epoch = time.time()
    for batch_idx, inputs in enumerate(adapt_loader):
      t0 = time.time()
      inputs = {key: value.cuda(non_blocking=True).detach() for key, value in inputs.items()}
      replay = None
      if er_mode:
        er = train_val_dataset[step % len(train_val_dataset)]           # a "random" pair of the training domain
        replay = (er[left_key].cuda().unsqueeze(0), er[right_key].cuda().unsqueeze(0), er[gt_key].cuda().unsqueeze(0))
      result = loop.process(inputs[left_key], inputs[right_key], batch_idx, replay=replay)
      outputs = result["outputs"]

      if (step % opt.log_frequency) == 0 and step > 0:
        torch.cuda.synchronize()
        elapsed_this_batch = time.time() - t0
        metrics = {}
        if gt_key in inputs:
          gt_disp = inputs[gt_key]
          metrics["EPE"] = torch.abs(gt_disp - outputs["pred_disp_l/{}".format(s)])[gt_disp > 0].mean()
        losses = {"Monodepth/total_loss": result["loss"], "fcs/raw": result["fcs"], "fcs/smoothed": result["fcs_smoothed"]}
        if result.get("replay_loss") is not None:
          losses["Replay/total_loss"] = result["replay_loss"]
        if result.get("proxy_loss") is not None:
          pixels = float(inputs[left_key].shape[0] * inputs[left_key].shape[-2] * inputs[left_key].shape[-1])
          losses.update({"Proxy/loss": result["proxy_loss"], "Proxy/epe": result["proxy_epe"], "Proxy/bad": result["proxy_bad"],
                         "Proxy/density": result["proxy_count"] / pixels})
        log_scalars(adapt_writer, metrics, losses, opt.batch_size / elapsed_this_batch, epoch, step)
        log_images(adapt_writer, inputs, outputs, step)
      step += 1

      mid_epoch_eval = opt.eval_hz > 0 and step % opt.eval_hz == 0
      end_epoch_eval = opt.eval_hz <= 0 and batch_idx == len(adapt_loader) - 1
      if mid_epoch_eval or end_epoch_eval:
        print("=============== MID-ADAPTATION EVALUATION (step {}) ==================".format(step))
        loop.sync()                     # gradient_updates and the optimizer's step count from the device (captured loop)
        if adapt_writer is not None:
          adapt_writer.add_scalar("GRADIENT_UPDATES", loop.gradient_updates, step)
        metrics_adapt = evaluate(feature_net, stereo_net, adapt_val_loader, opt)
        log_scalars(adapt_writer, metrics_adapt, {}, 0, epoch, step)
        metrics_train = evaluate(feature_net, stereo_net, train_val_loader, opt)
        log_scalars(train_writer, metrics_train, {}, 0, epoch, step)
        save_models(feature_net, stereo_net, adapter.optimizer, log_path, step)
        append_trial_row(trials_path, trial_index, step, metrics_adapt, metrics_train, loop.gradient_updates)
        print("Wrote data to {} (step={})".format(trials_path, step))
      if opt.num_steps > 0 and step >= opt.num_steps:
        break
    torch.cuda.synchronize()
    elapsed_epoch = time.time() - t0_epoch
    print("Finished {} adaptation steps in {:.02f}s ({:.02f} examples/s)".format(
        batch_idx + 1, elapsed_epoch, (batch_idx + 1) / elapsed_epoch))
  loop.sync()
  return loop


if __name__ == "__main__":
  print("\nStarting adaptation ...")
  adapt(TrainOptions().parse())
  print("Done with adaptation!")
