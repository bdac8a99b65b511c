"""The classical baseline beside evaluate_model.py: semi-global matching (adaptive_stereo.sgm) over a split, scored as
train.evaluate scores the network, so that the figures can be put side by side.

  python sgm_baseline.py --dataset_path ... --dataset_name KittiStereo2015 --split ... --subsplit val --height 320 --width 960
  python sgm_baseline.py ... --proxy          additionally the whole ProxyLabeler (left-right check, speckle filter)
  python sgm_baseline.py ... --median 1       additionally the matcher's left view after a (2R + 1)^2 median (adaptive_stereo.smooth),
                                              and with --proxy the labeler runs that median in front of its left-right check

Printed and returned per stage: EPE and D1_all_{2,3,4,5}px of train.disparity_metrics over the pixels that have ground truth AND a
kept code (the kernel counts gt > 0, so it is handed gt * kept), averaged per batch as train.evaluate averages, and "density":
kept pixels with ground truth over pixels with ground truth.  The matcher's parameters are the customary ones, not tuned.
"""
import argparse

import torch
from torch.utils.data import DataLoader

from adaptive_stereo.sgm import ProxyLabeler, SemiGlobalMatcher
from adaptive_stereo.smooth import DisparitySmoother
from evaluate_model import add_dataset_flags, make_dataset
from train import disparity_metrics


class _Score(object):
  """the running figures of one stage"""

  def __init__(self):
    self.rows, self.kept, self.labelled = [], [], []

  def add(self, disp, code, gt):
    has_gt = gt > 0
    kept = has_gt & (code == 0)
    self.rows.append(disparity_metrics(disp, gt * kept.float()))
    self.kept.append(kept.sum())
    self.labelled.append(has_gt.sum())

  def result(self):
    m = torch.stack(self.rows).mean(dim=0).cpu() if self.rows else torch.zeros(5)
    labelled = int(torch.stack(self.labelled).sum()) if self.labelled else 0
    density = float(torch.stack(self.kept).sum()) / labelled if labelled else 0.0
    return {"EPE": float(m[0]), "D1_all_2px": float(m[1]), "D1_all_3px": float(m[2]), "D1_all_4px": float(m[3]),
            "D1_all_5px": float(m[4]), "density": density}


def evaluate_sgm(batches, opt):
  """batches: an iterable of collated samples {"color_l/0", "color_r/0", "gt_disp_l/0"} (a DataLoader, or a list of dicts).
  -> {"sgm": figures} and, with opt.proxy, {"proxy": figures}, with opt.median {"sgm_median": figures}.  The matchers are kept per
  batch shape (the last batch of a split may be smaller)."""
  matchers, medians, scores = {}, {}, {"sgm": _Score()}
  if opt.proxy:
    scores["proxy"] = _Score()
  if opt.median:
    scores["sgm_median"] = _Score()
  params = dict(maxdisp=opt.maxdisp, p1=opt.p1, p2=opt.p2, paths=opt.paths, uniqueness=opt.uniqueness)
  with torch.no_grad():
    for inputs in batches:
      left, right = inputs["color_l/0"].cuda().float().contiguous(), inputs["color_r/0"].cuda().float().contiguous()
      gt = inputs["gt_disp_l/0"].cuda().float().contiguous()
      B, C, H, W = left.shape
      if (B, C, H, W) not in matchers:
        if opt.proxy:
          labeler = ProxyLabeler(H, W, batch=B, channels=C, tol_abs=opt.lr_tol, max_diff=opt.speckle_diff, max_size=opt.speckle_size,
                                 median_radius=opt.median, device=left.device, **params)
          matchers[(B, C, H, W)] = (labeler.matcher, labeler)
        else:
          matchers[(B, C, H, W)] = (SemiGlobalMatcher(H, W, batch=B, channels=C, device=left.device, **params), None)
      matcher, labeler = matchers[(B, C, H, W)]
      if labeler is not None:                                            # the chain runs the matcher itself (fill NaN)
        labels, code, _ = labeler(left, right)
        scores["proxy"].add(labels, code, gt)
        res = matcher.result()
        scores["sgm"].add(torch.nan_to_num(res.disp_l, nan=0.0), res.code_l, gt)
      else:
        res = matcher(left, right, fill=0.0)
        scores["sgm"].add(res.disp_l, res.code_l, gt)
      if opt.median:                                                     # the matcher's left view, gated by its own code map
        if (B, H, W) not in medians:
          medians[(B, H, W)] = DisparitySmoother(H, W, batch=B, radius=opt.median, device=left.device)
        sm = medians[(B, H, W)](res.disp_l, code_in=res.code_l)
        scores["sgm_median"].add(torch.nan_to_num(sm.disp, nan=0.0), sm.code, gt)
  return {name: score.result() for name, score in scores.items()}


def main(opt):
  dataset, workers = make_dataset(opt)
  loader = DataLoader(dataset, opt.batch_size, False, num_workers=workers, pin_memory=True, drop_last=False)
  figures = evaluate_sgm(loader, opt)
  print("semi-global matching (%d paths, P1 %d, P2 %d, uniqueness %d, %d disparities):" % (opt.paths, opt.p1, opt.p2, opt.uniqueness,
                                                                                          opt.maxdisp), figures["sgm"])
  if opt.median:
    print("... after a %d x %d median:" % (2 * opt.median + 1, 2 * opt.median + 1), figures["sgm_median"])
  if opt.proxy:
    print("proxy labels (left-right check within %g px, speckles of at most %d pixels):" % (opt.lr_tol, opt.speckle_size),
          figures["proxy"])
  return figures


def make_parser():
  p = argparse.ArgumentParser(description="Semi-global matching over a split: the classical baseline beside evaluate_model.py")
  add_dataset_flags(p)
  p.add_argument("--maxdisp", type=int, default=192, help="disparities searched, 1 .. 256")
  p.add_argument("--p1", type=int, default=10, help="penalty of a disparity step of one along a path")
  p.add_argument("--p2", type=int, default=120, help="penalty of a larger step, p1 .. 255")
  p.add_argument("--paths", type=int, default=8, choices=[4, 8])
  p.add_argument("--uniqueness", type=int, default=5, help="margin in per cent of the winner over every non-neighbour, 0 .. 99")
  p.add_argument("--proxy", action="store_true", default=False, help="also the whole ProxyLabeler: left-right check and speckle filter")
  p.add_argument("--lr_tol", type=float, default=1.0, help="--proxy: the left-right check's tolerance in pixels of disparity")
  p.add_argument("--speckle_size", type=int, default=200, help="--proxy: components of at most this many pixels are speckles")
  p.add_argument("--speckle_diff", type=float, default=1.0,
                 help="--proxy: neighbours at most this far apart in disparity belong to one component")
  p.add_argument("--median", type=int, default=0,
                 help="also the matcher after a (2R + 1)^2 median, 1 .. 7; with --proxy the labeler runs it before its check (0: off)")
  return p


if __name__ == "__main__":
  main(make_parser().parse_args())
