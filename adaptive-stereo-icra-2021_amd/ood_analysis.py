"""Calibrates --ood_threshold for a model: the compute of the reference's evaluation/ood_analysis.py (--save, --histogram,
--pr) without its plots.  Runs the train domain and a novel domain through the network in eval mode, keeps one feature-contrast
score per image (adaptive_stereo.ood: one launch per batch, one read-back per domain), and writes

  <output_folder>/train_fcs.pt, novel_fcs.pt   the max-minus-mean scores, as the reference saves them
                                               (train_<score>.pt, novel_<score>.pt for another --score)
  <output_folder>/ood.json                     score (the --score analysed), mu, sigma, threshold, n, the precision/recall
                                               sweep and the two histograms

  python ood_analysis.py --load_weights_folder W --stereonet_k 4 \\
      --train_dataset_path P --train_dataset_name VirtualKitti --train_split virtual_kitti_clone \\
      --novel_dataset_path Q --novel_dataset_name KittiRaw --novel_split kitti_raw_city_adapt --percentile 0.05

--score picks the per-image score: fcs_mean (the default, max-minus-mean), fcs_median (max-minus-median), or the entropy of the
left image's intensities (entropy_gray) or of their horizontal differences (entropy_grad), which need no network pass and no
weights (adaptive_stereo.utils.entropy).
"""
import argparse
import json
import os
import random


SCORES = {"fcs_mean": ("fcs", 0), "fcs_median": ("fcs", 1), "entropy_gray": ("entropy", 0), "entropy_grad": ("entropy", 1)}


def parse(args=None):
  p = argparse.ArgumentParser(description="FCS scores of two domains, the OOD threshold and its precision/recall evidence")
  p.add_argument("--height", type=int, default=320)
  p.add_argument("--width", type=int, default=960)
  p.add_argument("--load_weights_folder", default=None, type=str, help="folder with feature_net.pth and stereo_net.pth")
  p.add_argument("--stereonet_k", type=int, default=4, choices=[3, 4], help="the cost volume downsampling factor")
  p.add_argument("--stereonet_input_scale", type=int, default=0)
  p.add_argument("--batch_size", type=int, default=32)
  p.add_argument("--percentile", type=float, default=0.05, help="the threshold is this percentile of the fitted normal")
  for domain in ("train", "novel"):
    p.add_argument("--%s_dataset_path" % domain, type=str, required=True)
    p.add_argument("--%s_dataset_name" % domain, type=str, required=True)
    p.add_argument("--%s_split" % domain, type=str, required=True)
    p.add_argument("--%s_subsplit" % domain, type=str, default="train")
  p.add_argument("--num_train", type=int, default=1000)
  p.add_argument("--num_novel", type=int, default=1000)
  p.add_argument("--num_workers", type=int, default=4)
  p.add_argument("--output_folder", type=str, default="ood")
  p.add_argument("--score", type=str, default="fcs_mean", choices=sorted(SCORES), help="the per-image score to analyse")
  opt = p.parse_args(args)
  if not (0.01 <= opt.percentile <= 0.99):
    p.error("--percentile must lie in [0.01, 0.99]")
  return opt


def main(args=None):
  opt = parse(args)
  import torch
  from torch.utils.data import DataLoader

  from adaptive_stereo import ood
  from adaptive_stereo.datasets.stereo_dataset import StereoDataset
  from adaptive_stereo.models.stereo_net import StereoNet, FeatureExtractorNetwork

  torch.manual_seed(123)
  random.seed(123)
  s = opt.stereonet_input_scale
  family, column = SCORES[opt.score]
  tag = "fcs" if opt.score == "fcs_mean" else opt.score
  if family == "fcs":
    feature_net = FeatureExtractorNetwork(opt.stereonet_k).cuda()
    stereo_net = StereoNet(opt.stereonet_k, 1, s).cuda()
    feature_net.load_state_dict(torch.load(os.path.join(opt.load_weights_folder, "feature_net.pth")), strict=True)
    stereo_net.load_state_dict(torch.load(os.path.join(opt.load_weights_folder, "stereo_net.pth")), strict=True)

  scores = {}
  for domain, num in (("train", opt.num_train), ("novel", opt.num_novel)):
    dataset = StereoDataset(getattr(opt, domain + "_dataset_path"), getattr(opt, domain + "_dataset_name"),
                            getattr(opt, domain + "_split"), opt.height, opt.width, getattr(opt, domain + "_subsplit"),
                            scales=[s], load_disp_left=False, load_disp_right=False)
    loader = DataLoader(dataset, opt.batch_size, shuffle=True, pin_memory=True, drop_last=False, num_workers=opt.num_workers)
    if family == "fcs":
      both = ood.collect_scores(feature_net, stereo_net, loader, num, input_scale=s)
    else:
      both = ood.collect_image_entropy(loader, num, input_scale=s)
    scores[domain] = both[:, column].cpu()
    print("{}: {} images, {} {:.4f} .. {:.4f}".format(domain, len(scores[domain]), "FCS" if tag == "fcs" else opt.score,
                                                      float(scores[domain].min()), float(scores[domain].max())))

  os.makedirs(opt.output_folder, exist_ok=True)
  torch.save(scores["train"], os.path.join(opt.output_folder, "train_%s.pt" % tag))
  torch.save(scores["novel"], os.path.join(opt.output_folder, "novel_%s.pt" % tag))
  threshold, mu, sigma = ood.ood_threshold(scores["train"], opt.percentile)
  pr = ood.precision_recall(scores["train"], scores["novel"])
  recall_fixed, precision_fixed = ood.strictly_decreasing_precision(pr["precision"], pr["recall"])
  edges, density_train, density_novel = ood.fcs_histogram(scores["train"], scores["novel"])
  result = dict(score=opt.score, mu=mu, sigma=sigma, threshold=threshold, percentile=opt.percentile,
                n=dict(train=len(scores["train"]), novel=len(scores["novel"])),
                precision_recall={k: v.tolist() for k, v in pr.items()},
                precision_recall_monotone=dict(recall=recall_fixed.tolist(), precision=precision_fixed.tolist()),
                histogram=dict(edges=edges.tolist(), train=density_train.tolist(), novel=density_novel.tolist()))
  with open(os.path.join(opt.output_folder, "ood.json"), "w") as f:
    json.dump(result, f, indent=1)
  print("--ood_threshold {:.4f}   (mu {:.4f}, sigma {:.4f}, percentile {})".format(threshold, mu, sigma, opt.percentile))
  print("Saved to", opt.output_folder)


if __name__ == "__main__":
  main()
