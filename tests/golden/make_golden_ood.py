"""Generates tests/golden/ood_fcs.npz by running the REFERENCE's own feature-contrast functions.

Run in the build container only (needs /root/reference; the GPU box never has it):

    python tests/golden/make_golden_ood.py

What it does: imports feature_contrast_mean and feature_contrast_median from the reference's
adaptive_stereo/utils/feature_contrast.py (namespace package, cwd-independent) and runs them on the CPU over the seeded volumes
of tests/ood_ref.py (SHAPES x GAINS, with the planted pixels: all D values equal, the maximum twice, ties across the median
rank, zeros of both signs, one NaN).  The volumes are not stored: ood_ref.make_volume regenerates them from numpy's frozen
legacy generator, and a checksum of each is stored to prove it.  Both maps are stored whole.

It also stores a seeded set of 64 per-image scores with the thresholds that the reference's formula (plot_histogram,
evaluation/ood_analysis.py:203-204: torch's fp32 mean, the square root of torch's unbiased var, scipy.stats.norm.ppf) gives
for it at three percentiles; that script itself imports seaborn and matplotlib at the top and is not imported here.
No reference source text is stored in the fixture — only numeric arrays.
"""
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = "/root/reference"
sys.path.insert(0, os.path.dirname(HERE))
import ood_ref                                                                      # noqa: E402

sys.path.insert(0, REFERENCE)
from adaptive_stereo.utils import feature_contrast as ref_fc                        # noqa: E402

assert ref_fc.__file__.startswith(REFERENCE)

PERCENTILES = [0.01, 0.05, 0.5]


def main():
  import scipy.stats as stats
  store = {}
  for shape in ood_ref.SHAPES:
    for gain in ood_ref.GAINS:
      vol = ood_ref.make_volume(shape, gain)
      t = torch.from_numpy(vol)
      name = ood_ref.case_name(shape, gain)
      store["check__" + name] = ood_ref.checksum(vol)
      store["mean__" + name] = ref_fc.feature_contrast_mean(t).numpy()
      store["median__" + name] = ref_fc.feature_contrast_median(t).numpy()
  scores = torch.from_numpy((12.0 + 1.5 * np.random.RandomState(2021).standard_normal(64)).astype(np.float32))
  mu, sigma = scores.mean(), math.sqrt(scores.var())
  store["scores"] = scores.numpy()
  store["percentiles"] = np.array(PERCENTILES, dtype=np.float64)
  store["thresholds"] = np.array([float(stats.norm.ppf(p, loc=mu, scale=sigma)) for p in PERCENTILES], dtype=np.float64)
  store["meta"] = np.array("torch %s numpy %s" % (torch.__version__, np.__version__))
  path = os.path.join(HERE, "ood_fcs.npz")
  np.savez_compressed(path, **store)
  print("%s: %d arrays, %.1f KB" % (path, len(store), os.path.getsize(path) / 1e3))


if __name__ == "__main__":
  main()
