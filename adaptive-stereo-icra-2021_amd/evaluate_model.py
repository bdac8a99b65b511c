"""The reference's evaluate_model.py with its flags, on this package: saved predictions, per-frame images, metrics.

  --mode save      every "pred_disp" output of the network per sample as <weights>/outputs/<split>/<key with / as _>/<index>.pt
                   (evaluate_model.py:16-20, 34-70)
  --mode video     per frame left_#####.png, gt_#####.png (inferno, 0 .. 0.6 * 192) and pred_#####.png under the output folder's
                   video/, written through PIL from images painted on the device; the per-frame EPE is printed and written to
                   epe.csv.  The reference's text overlay needs OpenCV and is left out.
  --mode playback  needs a display and OpenCV windows: raises.
  --mode eval      does nothing in the reference; here it prints train.evaluate()'s metrics.
  --lr_check       (not in the reference; default off, nothing changes without it) predicts both views in one pass and checks them
                   against each other (adaptive_stereo.consistency).  save: additionally pred_disp_r/*, lr_code_l/0 (uint8: 0
                   consistent, 1 occluded, 2 mismatch, 3 out of view, 4 bad input) and pred_disp_l_filled/0.  eval: additionally the
                   metrics over the ground-truth pixels the check keeps, and the share of pixels kept.
  --post_filter    (not in the reference; default off, nothing changes without it) runs the discontinuity check and the speckle
                   filter on the left disparity (adaptive_stereo.disp_filter; --edge_tol, --speckle_diff, --speckle_size), alone
                   or on what --lr_check kept.  save: additionally filter_code_l/0 (uint8: the codes above, 5 discontinuity,
                   6 speckle), and with --lr_check pred_disp_l_filled/0 is filled from the combined code.  eval: additionally
                   the metrics over the ground-truth pixels the filter keeps, and the share of pixels kept.
  --smooth_radius R  (not in the reference; default 0: off, nothing changes without it) --mode eval: additionally EPE and D1 of the
                   left disparity after the weighted median of adaptive_stereo.smooth over a (2R + 1)^2 window, R 1 .. 7, beside
                   the figures above.  --smooth_sigma S guides it by the left image (S in units of the image's range; without it
                   the plain median); --smooth_fill lets it fill what --lr_check / --post_filter rejected, and the density (pixels
                   with ground truth that hold a value, over pixels with ground truth) is reported too.

Each mode is a function over a dataset-like iterable of {"color_l/0", "color_r/0", "gt_disp_l/0"} samples.
"""
import argparse
import csv
import os

import torch
from torch.utils.data import DataLoader

import adaptive_stereo.utils.path_utils as paths
from adaptive_stereo.utils.visualization import DisparityPainter
from train import disparity_metrics, evaluate, process_batch

VIDEO_CMAP, VIDEO_VMIN, VIDEO_VMAX = "inferno", 0, 0.6 * 192


def get_save_filename(save_folder, outputs_key, index):
  """<save_folder>/<key with / as _>/<index, four digits>.pt; the key's folder is created."""
  folder = os.path.join(save_folder, "_".join(outputs_key.split("/")))
  os.makedirs(folder, exist_ok=True)
  return os.path.join(folder, "%04d.pt" % index)


class _BothViews(object):
  """--lr_check: both views of a batch and their check; the buffers are kept per batch shape (the last batch may be smaller)."""

  def __init__(self, feature_net, stereo_net):
    if stereo_net.input_scale != 0:
      raise ValueError("--lr_check: the check runs on pred_disp_{l,r}/0; a StereoNet with input_scale %r has none"
                       % (stereo_net.input_scale,))
    self.feature_net, self.stereo_net, self._checkers = feature_net, stereo_net, {}

  def __call__(self, left, right):
    """-> (outputs with _l and _r keys, LRCheck, the left disparity filled)"""
    from adaptive_stereo.consistency import predict_disparity_leftright
    left, right = left.float().contiguous(), right.float().contiguous()
    outputs = predict_disparity_leftright(self.feature_net, self.stereo_net, left, right, output_cost_volume=True)
    disp_l = outputs["pred_disp_l/0"].contiguous()
    lrc = self.checker(disp_l)
    chk = lrc.check(disp_l, outputs["pred_disp_r/0"])
    return outputs, chk, lrc.fill(disp_l, chk.code_l)

  def checker(self, disp):
    """the LeftRightConsistency of a batch of maps [B,1,H,W]"""
    from adaptive_stereo.consistency import LeftRightConsistency
    B, _, H, W = disp.shape
    if (B, H, W) not in self._checkers:
      self._checkers[(B, H, W)] = LeftRightConsistency(H, W, batch=B, device=disp.device)
    return self._checkers[(B, H, W)]


class _PostFilter(object):
  """--post_filter: the DisparityFilter of a batch shape (the last batch may be smaller), with the flags' thresholds."""

  def __init__(self, opt):
    self.edge_tol, self.max_diff, self.max_size, self._filters = opt.edge_tol, opt.speckle_diff, opt.speckle_size, {}

  def __call__(self, disp, code_in=None):
    """-> DispFilter of the left disparity [B,1,H,W], on what code_in (the left-right check's code_l, or None) kept"""
    from adaptive_stereo.disp_filter import DisparityFilter
    key = tuple(disp.shape)
    if key not in self._filters:
      self._filters[key] = DisparityFilter(key[2], key[3], batch=key[0], tol_abs=self.edge_tol, max_diff=self.max_diff,
                                           max_size=self.max_size, device=disp.device)
    return self._filters[key](disp, code_in)


def save_outputs(feature_net, stereo_net, batches, save_folder, batch_size, opt=None, lr_check=False, post_filter=None):
  """batches: an iterable of collated samples (a DataLoader, or a list of dicts of [b,...] tensors).  Returns the number of
  samples written per key.  post_filter: a _PostFilter, or None."""
  feature_net.eval(); stereo_net.eval()
  written = 0
  both = _BothViews(feature_net, stereo_net) if lr_check else None
  with torch.no_grad():
    for i, inputs in enumerate(batches):
      left, right = inputs["color_l/0"].cuda(), inputs["color_r/0"].cuda()
      if both is not None:
        outputs, chk, filled = both(left, right)
        outputs = dict(outputs)
        outputs["lr_code_l/0"], outputs["pred_disp_l_filled/0"] = chk.code_l, filled
      else:
        outputs = process_batch(feature_net, stereo_net, left, right, opt, output_cost_volume=True)
      if post_filter is not None:
        outputs = dict(outputs)
        disp_l = outputs["pred_disp_l/0"].float().contiguous()
        filt = post_filter(disp_l, chk.code_l if both is not None else None)
        outputs["filter_code_l/0"] = filt.code
        if both is not None:                                         # the fill from the combined code, into a buffer of its own
          outputs["pred_disp_l_filled/0"] = both.checker(disp_l).fill(disp_l, filt.code, out=torch.empty_like(disp_l))
      for key in outputs:
        if "pred_disp" in key or key.startswith("lr_code") or key.startswith("filter_code"):
          for j in range(len(outputs[key])):
            torch.save(outputs[key][j].detach().cpu().clone(), get_save_filename(save_folder, key, batch_size * i + j))
      written += left.shape[0]
      total = " of %d" % len(batches) if hasattr(batches, "__len__") else ""
      print("saved batch %d%s (%d samples)" % (i + 1, total, written), flush=True)
  return written


def evaluate_lr_check(feature_net, stereo_net, val_loader):
  """{"EPE", "D1_all_{2,3,4,5}px"} of train.disparity_metrics over the ground-truth pixels whose left-right code is 0 (the kernel
  counts gt > 0, so it is handed gt * valid_l), averaged per batch as train.evaluate averages, and "kept": the share of all
  pixels with code 0."""
  feature_net.eval(); stereo_net.eval()
  both = _BothViews(feature_net, stereo_net)
  rows, kept, pixels = [], [], 0
  with torch.no_grad():
    for inputs in val_loader:
      left, right = inputs["color_l/0"].cuda(), inputs["color_r/0"].cuda()
      gt = inputs["gt_disp_l/0"].cuda().float()
      outputs, chk, _ = both(left, right)
      rows.append(disparity_metrics(outputs["pred_disp_l/0"], gt * chk.valid_l))
      kept.append(chk.counts[:, 0, 0].sum().clone())               # the buffers are overwritten by the next batch
      pixels += gt.numel()
    m = torch.stack(rows).mean(dim=0).cpu() if rows else torch.zeros(5)
    share = float(torch.stack(kept).sum()) / pixels if pixels else 0.0
  return {"EPE": float(m[0]), "D1_all_2px": float(m[1]), "D1_all_3px": float(m[2]), "D1_all_4px": float(m[3]),
          "D1_all_5px": float(m[4]), "kept": share}


def evaluate_post_filter(feature_net, stereo_net, val_loader, opt, lr_check=False):
  """evaluate_lr_check's figures over the ground-truth pixels the post-filter keeps (code 0 after the edge check and the speckle
  pass; with lr_check on what the left-right check kept): {"EPE", "D1_all_{2,3,4,5}px", "kept"}."""
  feature_net.eval(); stereo_net.eval()
  both = _BothViews(feature_net, stereo_net) if lr_check else None
  post = _PostFilter(opt)
  rows, kept, pixels = [], [], 0
  with torch.no_grad():
    for inputs in val_loader:
      left, right = inputs["color_l/0"].cuda(), inputs["color_r/0"].cuda()
      gt = inputs["gt_disp_l/0"].cuda().float()
      if both is not None:
        outputs, chk, _ = both(left, right)
      else:
        outputs, chk = process_batch(feature_net, stereo_net, left, right, opt), None
      disp_l = outputs["pred_disp_l/0"].float().contiguous()
      filt = post(disp_l, chk.code_l if chk is not None else None)
      rows.append(disparity_metrics(disp_l, gt * filt.valid))
      kept.append(filt.counts[:, 0].sum().clone())                   # the buffers are overwritten by the next batch
      pixels += gt.numel()
    m = torch.stack(rows).mean(dim=0).cpu() if rows else torch.zeros(5)
    share = float(torch.stack(kept).sum()) / pixels if pixels else 0.0
  return {"EPE": float(m[0]), "D1_all_2px": float(m[1]), "D1_all_3px": float(m[2]), "D1_all_4px": float(m[3]),
          "D1_all_5px": float(m[4]), "kept": share}


class _Smoother(object):
  """--smooth_radius: the DisparitySmoother of a batch shape (the last batch may be smaller), with the flags' settings."""

  def __init__(self, opt):
    self.radius, self.sigma, self.fill, self._smoothers = opt.smooth_radius, opt.smooth_sigma, opt.smooth_fill, {}

  def __call__(self, disp, left, code_in=None):
    """-> Smoothed of the left disparity [B,1,H,W], guided by `left` when --smooth_sigma is given, on what code_in kept"""
    from adaptive_stereo.smooth import DisparitySmoother
    key = tuple(disp.shape) + (left.shape[1],)
    if key not in self._smoothers:
      self._smoothers[key] = DisparitySmoother(key[2], key[3], batch=key[0], radius=self.radius, sigma_color=self.sigma,
                                               channels=key[4], fill=self.fill, device=disp.device)
    return self._smoothers[key](disp, left.float().contiguous() if self.sigma is not None else None, code_in)


def evaluate_smoothing(feature_net, stereo_net, val_loader, opt):
  """The figures of the left disparity before and after the weighted median, over the same pixels where nothing is filled:
  {"raw": {...}, "smoothed": {...}}, each {"EPE", "D1_all_{2,3,4,5}px", "density"} over the ground-truth pixels that hold a value
  (code 0; before: of --lr_check / --post_filter where given, else every usable pixel), "density" being those pixels over the
  pixels with ground truth."""
  feature_net.eval(); stereo_net.eval()
  both = _BothViews(feature_net, stereo_net) if opt.lr_check else None
  post = _PostFilter(opt) if opt.post_filter else None
  smoother = _Smoother(opt)
  rows = {"raw": [], "smoothed": []}
  kept = {"raw": [], "smoothed": []}
  labelled = []
  with torch.no_grad():
    for inputs in val_loader:
      left, right = inputs["color_l/0"].cuda(), inputs["color_r/0"].cuda()
      gt = inputs["gt_disp_l/0"].cuda().float()
      if both is not None:
        outputs, chk, _ = both(left, right)
        code = chk.code_l
      else:
        outputs, code = process_batch(feature_net, stereo_net, left, right, opt), None
      disp_l = outputs["pred_disp_l/0"].float().contiguous()
      if post is not None:
        code = post(disp_l, code).code
      sm = smoother(disp_l, left, code)
      usable = (disp_l >= 0) & ~torch.isinf(disp_l)
      before = usable if code is None else usable & (code == 0)
      has_gt = gt > 0
      for name, disp, ok in (("raw", disp_l, before), ("smoothed", sm.disp, sm.code == 0)):
        ok = ok & has_gt
        rows[name].append(disparity_metrics(torch.where(ok, disp, torch.zeros_like(disp)), gt * ok.float()))
        kept[name].append(ok.sum())
      labelled.append(has_gt.sum())
  figures = {}
  n = int(torch.stack(labelled).sum()) if labelled else 0
  for name in rows:
    m = torch.stack(rows[name]).mean(dim=0).cpu() if rows[name] else torch.zeros(5)
    figures[name] = {"EPE": float(m[0]), "D1_all_2px": float(m[1]), "D1_all_3px": float(m[2]), "D1_all_4px": float(m[3]),
                     "D1_all_5px": float(m[4]), "density": float(torch.stack(kept[name]).sum()) / n if n else 0.0}
  return figures


def frame_epe(pred, gt):
  """Mean |pred - gt| over gt > 0 of one frame (evaluate_model.py:110), a Python float."""
  valid = gt > 0
  return float((pred - gt).abs()[valid].mean())


def write_video_frames(samples, save_folder, video_folder, frames=-1):
  """samples: an iterable of single samples (tensors [C,H,W]); the predictions are the files save_outputs wrote.  Returns the
  list of per-frame EPEs."""
  from PIL import Image
  os.makedirs(video_folder, exist_ok=True)
  painter, epes = None, []
  with open(os.path.join(video_folder, "epe.csv"), "w", newline="") as f:
    rows = csv.writer(f)
    rows.writerow(["frame", "epe"])
    for i, inputs in enumerate(samples):
      if frames > 0 and i >= frames:
        break
      left = inputs["color_l/0"].cuda().float().contiguous()
      gt = inputs["gt_disp_l/0"].cuda().float().contiguous()
      pred = torch.load(get_save_filename(save_folder, "pred_disp_l/0", i)).cuda().float().contiguous()
      if painter is None:
        painter = DisparityPainter(gt.shape[-2], gt.shape[-1], batch=1, cmap=VIDEO_CMAP, vmin=VIDEO_VMIN, vmax=VIDEO_VMAX,
                                   order="rgb", out="u8", device=gt.device)          # PIL takes RGB
      epe = frame_epe(pred, gt)
      print("EPE:", epe)
      rows.writerow([i, "{:.6f}".format(epe)])
      epes.append(epe)
      for name, image in (("left", painter.rgb(left)[0].cpu()), ("gt", painter.paint(gt)[0].cpu()),
                          ("pred", painter.paint(pred)[0].cpu())):
        Image.fromarray(image.numpy()).save(os.path.join(video_folder, "{}_{:05d}.png".format(name, i)))
  return epes


def load_networks(opt):
  from adaptive_stereo.models.stereo_net import StereoNet, FeatureExtractorNetwork
  feature_net = FeatureExtractorNetwork(opt.stereonet_k).cuda()
  stereo_net = StereoNet(opt.stereonet_k, 1, 0).cuda()
  feature_net.load_state_dict(torch.load(os.path.join(opt.load_weights_folder, "feature_net.pth"), map_location="cpu"), strict=True)
  stereo_net.load_state_dict(torch.load(os.path.join(opt.load_weights_folder, "stereo_net.pth"), map_location="cpu"), strict=True)
  return feature_net, stereo_net


def make_dataset(opt):
  """-> (the evaluation dataset of the flags: no flip, no crop, left ground truth; the loader processes to use).  sgm_baseline.py
  evaluates on the same samples."""
  from adaptive_stereo.datasets.stereo_dataset import StereoDataset
  dataset = StereoDataset(opt.dataset_path, opt.dataset_name, opt.split, opt.height, opt.width, opt.subsplit, scales=opt.scales,
                          do_hflip=False, random_crop=False, load_disp_left=True, load_disp_right=False,
                          splits_path=opt.splits_path)
  return dataset, opt.batch_size if opt.num_workers is None else opt.num_workers


def main(opt):
  if opt.mode == "playback":
    raise RuntimeError("--mode playback opens OpenCV windows and needs a display; use --mode video and view the PNGs")
  save_folder = os.path.join(opt.load_weights_folder, "outputs", opt.split)
  os.makedirs(save_folder, exist_ok=True)
  dataset, workers = make_dataset(opt)
  if opt.mode == "save":
    feature_net, stereo_net = load_networks(opt)
    loader = DataLoader(dataset, opt.batch_size, False, num_workers=workers, pin_memory=True, drop_last=False)
    save_outputs(feature_net, stereo_net, loader, save_folder, opt.batch_size, opt, lr_check=opt.lr_check,
                 post_filter=_PostFilter(opt) if opt.post_filter else None)
  elif opt.mode == "video":
    write_video_frames(dataset, save_folder, paths.output_folder("video"), opt.frames)
  elif opt.mode == "eval":
    feature_net, stereo_net = load_networks(opt)
    opt.stereonet_input_scale = 0
    loader = DataLoader(dataset, opt.batch_size, False, num_workers=workers, pin_memory=True, drop_last=False)
    print(evaluate(feature_net, stereo_net, loader, opt))
    if opt.lr_check:
      print("left-right consistent pixels only:", evaluate_lr_check(feature_net, stereo_net, loader))
    if opt.post_filter:
      print("pixels the post-filter keeps%s:" % (" after the left-right check" if opt.lr_check else ""),
            evaluate_post_filter(feature_net, stereo_net, loader, opt, lr_check=opt.lr_check))
    if opt.smooth_radius:
      figures = evaluate_smoothing(feature_net, stereo_net, loader, opt)
      what = "plain median" if opt.smooth_sigma is None else "weighted median (sigma %g)" % opt.smooth_sigma
      print("before the %s of radius %d:" % (what, opt.smooth_radius), figures["raw"])
      print("after the %s of radius %d%s:" % (what, opt.smooth_radius, ", filling" if opt.smooth_fill else ""), figures["smoothed"])
  else:
    raise NotImplementedError()


def add_dataset_flags(p):
  """The flags make_dataset() reads, with the reference's defaults (sgm_baseline.py takes the same ones)."""
  p.add_argument("--dataset_path", type=str, help="root folder of the dataset")
  p.add_argument("--dataset_name", type=str, help="dataset loader to use")
  p.add_argument("--split", type=str, help="folder of split files")
  p.add_argument("--subsplit", choices=["train", "val", "test"], help="which lines file of the split")
  p.add_argument("--scales", type=int, nargs="+", default=[0], help="pyramid levels the dataset yields")
  p.add_argument("--batch_size", type=int, default=8)
  p.add_argument("--height", type=int, default=512, help="a multiple of 64")
  p.add_argument("--width", type=int, default=960, help="a multiple of 64")
  p.add_argument("--splits_path", default=None, type=str, help="folder of the split folders (default: the package's splits/)")
  p.add_argument("--num_workers", default=None, type=int, help="loader processes (default: the batch size, as the reference)")


def make_parser():
  """The reference's flags and defaults; the viewer flags (max_disp_viz, window_sf, wait, save_disp_as_image) are accepted and
  unused, as playback is."""
  p = argparse.ArgumentParser(description="Saved predictions, per-frame images and metrics of a trained StereoNet")
  p.add_argument("--mode", type=str, choices=["save", "playback", "eval", "video"])
  add_dataset_flags(p)
  p.add_argument("--load_weights_folder", default=None, type=str, help="folder holding feature_net.pth and stereo_net.pth")
  p.add_argument("--stereonet_k", type=int, default=3, choices=[3, 4], help="the cost volume is built at 1 / 2^k resolution")
  p.add_argument("--max_disp_viz", type=float, default=300)
  p.add_argument("--window_sf", type=float, default=1.5)
  p.add_argument("--wait", default=False, action="store_true")
  p.add_argument("--frames", default=-1, type=int, help="stop --mode video after this many frames (-1: all)")
  p.add_argument("--save_disp_as_image", action="store_true", default=False)
  p.add_argument("--lr_check", action="store_true", default=False,
                 help="predict both views and check them against each other (save: extra outputs; eval: extra metrics)")
  p.add_argument("--post_filter", action="store_true", default=False,
                 help="discontinuity check and speckle filter of the left disparity (save: extra output; eval: extra metrics)")
  p.add_argument("--edge_tol", type=float, default=1.0, help="--post_filter: a jump above this many pixels of disparity is an edge")
  p.add_argument("--speckle_size", type=int, default=200, help="--post_filter: components of at most this many pixels are speckles")
  p.add_argument("--speckle_diff", type=float, default=1.0,
                 help="--post_filter: neighbours at most this far apart in disparity belong to one component")
  p.add_argument("--smooth_radius", type=int, default=0,
                 help="eval: also the figures after a weighted median over a (2R + 1)^2 window, 1 .. 7 (0: off)")
  p.add_argument("--smooth_sigma", type=float, default=None,
                 help="--smooth_radius: guide the median by the left image, in units of its range (default: the plain median)")
  p.add_argument("--smooth_fill", action="store_true", default=False,
                 help="--smooth_radius: fill rejected pixels from their window; the density is reported")
  return p


if __name__ == "__main__":
  main(make_parser().parse_args())
