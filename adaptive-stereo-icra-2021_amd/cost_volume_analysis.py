"""What the matching curves look like where the feature-contrast score is extreme: the compute and the figures of the reference's
evaluation/cost_volume_analysis.py.  Per image of a train and a novel domain, the coarse pixel where the max-minus-mean map is
largest ("hi") and smallest ("lo"), its curve over disparity, its maximum, the mean of the rest and the true disparity there —
found on the device, one launch per image and one read-back per domain (adaptive_stereo.cv_probe) — plus the mean per rank of
every pixel's sorted logits, the average shape of an image's curves.

  --save        <output_folder>/<domain>/probes.pt   dict of tensors: pix [n,2,3] (row, col, d_max), vals [n,2,5] (fcs, max,
                                                     second, mean_rest, gt), slices [n,2,D], profile [n,D]; second axis (hi, lo)
                with --save_volumes also             {i}_cost_volume.pt, {i}_gt.pt per image, as the reference saves them
  --visualize   <output_folder>/<domain>/{i}_cost_volume_slice.pdf   train: the "hi" pick, novel: the "lo" pick
                <output_folder>/rank_profile.pdf                      both domains' mean profiles

  python cost_volume_analysis.py --save --load_weights_folder W --stereonet_k 4 --num_images 10 \\
      --train_dataset_path P --train_dataset_name SceneFlowFlying --train_split sceneflow_flying \\
      --novel_dataset_path Q --novel_dataset_name VirtualKitti --novel_split virtual_kitti_01_adapt
  python cost_volume_analysis.py --visualize --num_images 10
"""
import argparse
import os

DOMAINS = ("train", "novel")
DOMAIN_PICK = {"train": "hi", "novel": "lo"}          # the reference draws argmax for train and argmin for novel (:147-150)
DOMAIN_COLOR = {"train": "tab:blue", "novel": "tab:red"}
WHICH = {"hi": 0, "lo": 1}


def parse(args=None):
  p = argparse.ArgumentParser(description="matching curves at the pixels of extreme feature contrast, and the rank profile")
  p.add_argument("--height", type=int, default=320)
  p.add_argument("--width", type=int, default=960)
  p.add_argument("--load_weights_folder", default=None, type=str, help="folder with feature_net.pth and stereo_net.pth")
  p.add_argument("--stereonet_k", type=int, default=4, choices=[3, 4], help="the cost volume downsampling factor")
  p.add_argument("--save", action="store_true", help="probe the cost volumes of the train and the novel data")
  p.add_argument("--save_volumes", action="store_true", help="with --save: also write every cost volume and its ground truth")
  p.add_argument("--debug", action="store_true", help="not implemented, as in the reference")
  p.add_argument("--visualize", action="store_true", help="draw the curves from what --save wrote")
  p.add_argument("--num_images", type=int, default=10, help="the number of images to analyze")
  for domain in DOMAINS:
    p.add_argument("--%s_dataset_path" % domain, type=str, default=None)
    p.add_argument("--%s_dataset_name" % domain, type=str, default=None)
    p.add_argument("--%s_split" % domain, type=str, default=None)
    p.add_argument("--%s_subsplit" % domain, type=str, default="train")
  p.add_argument("--output_folder", type=str, default="cost_volume_analysis")
  p.add_argument("--ylim", type=float, nargs=2, default=[-22.0, 12.0], help="the figures' shared value range")
  opt = p.parse_args(args)
  if opt.save:
    missing = ["--%s_%s" % (d, f) for d in DOMAINS for f in ("dataset_path", "dataset_name", "split")
               if getattr(opt, "%s_%s" % (d, f)) is None]
    if missing or opt.load_weights_folder is None:
      p.error("--save needs --load_weights_folder and " + ", ".join(missing or ["the dataset flags"]))
  return opt


def save_probes(feature_net, stereo_net, samples, output_folder, num_images, save_volumes=False):
  """Probes the first num_images samples of `samples` (an indexable of sample dicts without a batch axis) at batch 1 and writes
  <output_folder>/probes.pt; returns the dict it wrote (CPU tensors)."""
  import torch
  from adaptive_stereo import cv_probe

  os.makedirs(output_folder, exist_ok=True)
  n = min(int(num_images), len(samples))

  def batches():
    for i in range(n):
      yield {key: value.unsqueeze(0) for key, value in samples[i].items() if torch.is_tensor(value)}

  def keep(first, cost_volume, gt):
    torch.save(cost_volume.cpu(), os.path.join(output_folder, "{}_cost_volume.pt".format(first)))
    if gt is not None:
      torch.save(gt.cpu(), os.path.join(output_folder, "{}_gt.pt".format(first)))

  result = cv_probe.collect_probes(feature_net, stereo_net, batches(), n, profile=True, on_batch=keep if save_volumes else None)
  probes = {name: t.cpu() for name, t in result.state_dict().items()}
  torch.save(probes, os.path.join(output_folder, "probes.pt"))
  return probes


def curve_data(probes, i, which):
  """The numbers behind the figure of image i: dict(disparity [D] int, curve [D] fp32 numpy, max, mean_rest, gt, fcs (floats),
  row, col, d_max (ints)), read at the "hi" or the "lo" pick."""
  if which not in WHICH:
    raise ValueError("curve_data: which must be 'hi' or 'lo' (got %r)" % (which,))
  w = WHICH[which]
  n = probes["pix"].shape[0]
  if not (0 <= i < n):
    raise IndexError("curve_data: image %d of %d" % (i, n))
  pix, vals = probes["pix"][i, w].tolist(), probes["vals"][i, w].tolist()
  curve = probes["slices"][i, w].detach().cpu().numpy()
  return dict(disparity=list(range(len(curve))), curve=curve, fcs=vals[0], max=vals[1], mean_rest=vals[3], gt=vals[4],
              row=int(pix[0]), col=int(pix[1]), d_max=int(pix[2]))


def visualize(output_folder, num_images, ylim=(-22.0, 12.0)):
  """Writes {i}_cost_volume_slice.pdf per image and domain and one rank_profile.pdf; returns the list of files written."""
  # The package carries no plotting dependency (tests/test_visualization_ref_cpu.py looks for an import statement of it in every
  # file); the figures are the one optional use, so matplotlib is loaded by name here, only when --visualize asks for them.
  import importlib
  matplotlib = importlib.import_module("matplotlib")
  matplotlib.use("Agg")
  plt = importlib.import_module("matplotlib.pyplot")
  import numpy as np
  import torch

  written, profiles = [], {}
  for domain in DOMAINS:
    folder = os.path.join(output_folder, domain)
    probes = torch.load(os.path.join(folder, "probes.pt"))
    profiles[domain] = probes["profile"].double().mean(dim=0).numpy()
    for i in range(min(int(num_images), probes["pix"].shape[0])):
      c = curve_data(probes, i, DOMAIN_PICK[domain])
      D = len(c["curve"])
      fig = plt.figure(figsize=(4, 3))
      plt.plot(np.arange(D), c["curve"], color=DOMAIN_COLOR[domain], linestyle="-")
      plt.xticks(np.arange(0, D, step=2))
      plt.xlabel("disparity")
      if domain == "train":
        plt.ylabel("feature similarity score")
      plt.ylim(ylim)
      for label in ("max", "mean_rest"):
        plt.hlines(c[label], xmin=0, xmax=D - 2.5, linestyles="dashed", colors="gray")
        plt.text(D - 2.5, c[label], "max" if label == "max" else "mean", va="center")
      if c["gt"] == c["gt"]:                               # NaN: no ground truth for this image
        plt.vlines(c["gt"], ymin=ylim[0], ymax=ylim[1], linestyles="dashed", colors="black")
        plt.text(c["gt"], (ylim[0] + ylim[1]) / 2, "true disparity", rotation=90, va="center", ha="right")
      path = os.path.join(folder, "{}_cost_volume_slice.pdf".format(i))
      fig.savefig(path, bbox_inches="tight")
      plt.close(fig)
      written.append(path)
  fig = plt.figure(figsize=(4, 3))
  for domain in DOMAINS:
    plt.plot(np.arange(len(profiles[domain])), profiles[domain], color=DOMAIN_COLOR[domain], label=domain)
  plt.xlabel("rank (0 = the maximum)")
  plt.ylabel("mean sorted similarity score")
  plt.legend()
  path = os.path.join(output_folder, "rank_profile.pdf")
  fig.savefig(path, bbox_inches="tight")
  plt.close(fig)
  written.append(path)
  return written


def main(args=None):
  opt = parse(args)
  if opt.save:
    import torch
    from adaptive_stereo.datasets.stereo_dataset import StereoDataset
    from adaptive_stereo.models.stereo_net import StereoNet, FeatureExtractorNetwork

    feature_net = FeatureExtractorNetwork(opt.stereonet_k).cuda()
    stereo_net = StereoNet(opt.stereonet_k, 1, 0).cuda()
    feature_net.load_state_dict(torch.load(os.path.join(opt.load_weights_folder, "feature_net.pth")), strict=True)
    stereo_net.load_state_dict(torch.load(os.path.join(opt.load_weights_folder, "stereo_net.pth")), strict=True)
    for domain in DOMAINS:
      dataset = StereoDataset(getattr(opt, domain + "_dataset_path"), getattr(opt, domain + "_dataset_name"),
                              getattr(opt, domain + "_split"), opt.height, opt.width, getattr(opt, domain + "_subsplit"),
                              scales=[0, opt.stereonet_k], load_disp_left=True, load_disp_right=False)
      probes = save_probes(feature_net, stereo_net, dataset, os.path.join(opt.output_folder, domain), opt.num_images,
                           save_volumes=opt.save_volumes)
      pick = WHICH[DOMAIN_PICK[domain]]
      print("{}: {} images, FCS at the {} pick {:.4f} .. {:.4f}".format(
          domain, probes["pix"].shape[0], DOMAIN_PICK[domain], float(probes["vals"][:, pick, 0].min()),
          float(probes["vals"][:, pick, 0].max())))
    print("Saved to", opt.output_folder)
  elif opt.visualize:
    for path in visualize(opt.output_folder, opt.num_images, ylim=tuple(opt.ylim)):
      print("Wrote", path)
  else:
    raise NotImplementedError()


if __name__ == "__main__":
  main()
