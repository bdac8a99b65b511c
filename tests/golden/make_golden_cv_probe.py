"""Generates tests/golden/cv_probe.npz by running the REFERENCE's own feature_contrast_mean and the steps of its
evaluation/cost_volume_analysis.py:82-90 on the seeded volumes of tests/cv_probe_ref.py.

Run in the build container only (needs /root/reference; the GPU box never has it):

    python tests/golden/make_golden_cv_probe.py

Per image of every case with D > 2 (for D <= 2 the reference's map is NaN, the mean of an empty slice, and the project's is 0 by
contract): fcs = feature_contrast_mean(volume); torch.argmax and torch.argmin of the flattened map; the slice at that pixel;
torch.sort(descending=True); sorted[0] and sorted[2:].mean().  Stored: the flattened picks, the two values, a checksum of the
regenerated volume.  The volumes are not stored (cv_probe_ref.make_case regenerates them).  That script itself imports seaborn
and pandas at the top and is not imported here.  No reference source text is stored in the fixture — only numeric arrays.

The reference's map (a mean of the sorted values) and the project's (an in-order sum minus the two largest) round differently,
so a pick is only a fixture where rounding cannot move it.  For every stored image and both extremes this script ASSERTS one of:
  * the gap between the extreme and the runner-up in the reference's map exceeds 100 times the rounding bound
    (D + 2) * 2^-24 * max_p sum_d |v| / (D - 2);
  * the tie is exact: both values are 0.0, or the case planted equal columns there;
  * the image holds a NaN.
A case that fails gets another seed, never a tolerance.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = "/root/reference"
sys.path.insert(0, os.path.dirname(HERE))
import cv_probe_ref as R                                                            # noqa: E402
import ood_ref                                                                      # noqa: E402

sys.path.insert(0, REFERENCE)
from adaptive_stereo.utils import feature_contrast as ref_fc                        # noqa: E402

assert ref_fc.__file__.startswith(REFERENCE)


def main():
  store, smallest_margin = {}, np.inf
  for name in R.STORED_NAMES:
    vol, gt, forced = R.make_case(name)
    B, D, H, W = vol.shape
    t = torch.from_numpy(vol)
    picks = np.zeros((B, 2), np.int64)
    maxes = np.zeros((B, 2), np.float32)
    means = np.zeros((B, 2), np.float32)
    for b in range(B):
      volume_b = t[b:b + 1]
      fcs = ref_fc.feature_contrast_mean(volume_b)
      bound = (D + 2) * 2.0 ** -24 * float(np.nanmax(np.abs(vol[b]).astype(np.float64).sum(axis=0))) / (D - 2)
      for which, arg in enumerate((torch.argmax, torch.argmin)):
        idx = int(arg(fcs.flatten()))
        srt = torch.sort(volume_b[0, :, idx // W, idx % W], descending=True)[0]
        picks[b, which] = idx
        maxes[b, which] = float(srt[0])
        means[b, which] = float(srt[2:].mean())
        # is this pick beyond the reach of rounding?
        flat = fcs.flatten().numpy().astype(np.float64)
        if np.isnan(flat).any():
          assert np.isnan(flat[picks[b, which]]) and not np.isnan(flat[:picks[b, which]]).any(), "not the first NaN pixel"
          continue
        if flat.size == 1:                                  # one pixel: nothing to choose between
          continue
        order = np.sort(flat)
        gap = order[-1] - order[-2] if which == 0 else order[1] - order[0]
        if gap == 0.0:
          assert flat[picks[b, which]] == 0.0 or (b, which) in forced, "%s image %d: an unplanted exact tie" % (name, b)
          assert picks[b, which] == int(np.flatnonzero(flat == flat[picks[b, which]])[0]), "not the first of the tied pixels"
        else:
          assert gap > 100.0 * bound, "%s image %d which %d: gap %.3e within 100 x bound %.3e: take another seed" % (
              name, b, which, gap, bound)
          smallest_margin = min(smallest_margin, gap / bound)
      for (fb, which), p in forced.items():
        if fb == b:
          assert picks[b, which] == p, "%s: the planted pick %d is not the reference's (%d)" % (name, p, picks[b, which])
    # the reference's picks are those of the project's own map everywhere
    mine = R.probe(vol)["p"]
    assert np.array_equal(mine, picks), "%s: picks differ from the restated map's: %s vs %s" % (name, mine.tolist(), picks.tolist())
    store["check__" + name] = ood_ref.checksum(vol)
    store["pick__" + name] = picks
    store["max__" + name] = maxes
    store["mean__" + name] = means
  store["meta"] = np.array("torch %s numpy %s" % (torch.__version__, np.__version__))
  path = os.path.join(HERE, "cv_probe.npz")
  np.savez_compressed(path, **store)
  print("%s: %d arrays, %.1f KB; smallest gap / bound %.0f" % (path, len(store), os.path.getsize(path) / 1e3, smallest_margin))


if __name__ == "__main__":
  main()
