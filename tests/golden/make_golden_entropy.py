"""Generates tests/golden/entropy.npz and tests/golden/entropy_bound.json by running the REFERENCE's own utils/entropy.py.

Run in the build container only (needs /root/reference; the GPU box never has it):

    python tests/golden/make_golden_entropy.py

The reference calls torch.histc on an int tensor, which no CPU build of torch accepts.  For integer-valued input histc on the
fp32 copy puts every value into the bin the integer path would (bin v for v in 0..255 over [0, 255]; bin
min((d + 255) * 256 // 510, 255) for d in -255..255 over [-255, 255]; both identities are asserted below against bincount
before anything is recorded), so torch.histc is wrapped to cast int tensors to fp32 and the reference's functions run as they are.

Stored per image: the input (fp32) and the reference's fp32 result(s): `gray__<name>` for every image, `grad__<name>` for the
2-D ones (the reference's gradient function asserts 2-D).  Images: the four of the reference's test/test_entropy.py (recorded
by running that test file itself with its entropy function wrapped, and stored under the names of its test methods), seeded
random [1,H,W], [3,H,W] and [H,W] images in [0, 1] with H, W in 5..65, and images in [-0.1, 1.2] so that values outside the
bins occur.  No reference source text is stored — only numeric arrays.

entropy_bound.json: how far the reference's fp32 sum lies from float32(the fp64 entropy of the same counts), in fp32 ulps, per
column over the non-exact images.  tests/test_entropy_ref_cpu.py asserts 2 x that figure.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = "/root/reference"
sys.path.insert(0, os.path.dirname(HERE))
import entropy_ref as R                                                             # noqa: E402

sys.path.insert(0, REFERENCE)
from adaptive_stereo.utils import entropy as ref_entropy                            # noqa: E402

assert ref_entropy.__file__.startswith(REFERENCE)

_histc = torch.histc


def histc_int_as_fp32(input, bins=100, min=0, max=0):
  if not input.is_floating_point():
    input = input.float()                   # exact: |value| < 2^24 for every image here
  return _histc(input, bins, min=min, max=max)


def check_identities():
  v = torch.arange(0, 256, dtype=torch.int32)
  assert torch.equal(histc_int_as_fp32(v, 256, min=0, max=255), torch.bincount(v, minlength=256).float())
  d = torch.arange(-255, 256, dtype=torch.int32)
  want = torch.bincount(torch.clamp((d.long() + 255) * 256 // 510, max=255), minlength=256).float()
  assert torch.equal(histc_int_as_fp32(d, 256, min=-255, max=255), want)
  for one in d.tolist():                    # value by value: no bin borrows from a neighbour
    got = histc_int_as_fp32(torch.tensor([one], dtype=torch.int32), 256, min=-255, max=255)
    assert int(got.argmax()) == min((one + 255) * 256 // 510, 255) and float(got.sum()) == 1.0


def reference_test_images():
  """Runs the reference's test/test_entropy.py (its `.cuda()` made a no-op: this machine has no GPU) with the function it
  imports wrapped to keep what it is given: {test method name: image}.  The test's own assertions run too."""
  import importlib.util
  import unittest
  sys.path.insert(0, os.path.join(REFERENCE, "adaptive_stereo"))          # the test file imports `utils.entropy`
  spec = importlib.util.spec_from_file_location("reference_test_entropy", os.path.join(REFERENCE, "test", "test_entropy.py"))
  module = importlib.util.module_from_spec(spec)
  cuda = torch.Tensor.cuda
  torch.Tensor.cuda = lambda self, *a, **k: self
  try:
    spec.loader.exec_module(module)
    wrapped, seen = module.grayscale_shannon_entropy, []
    module.grayscale_shannon_entropy = lambda img: (seen.append(img.clone()), wrapped(img))[1]
    out = {}
    for name in unittest.TestLoader().getTestCaseNames(module.EntropyTest):
      del seen[:]
      result = unittest.TestResult()
      module.EntropyTest(name).run(result)
      assert result.wasSuccessful() and len(seen) == 1, (name, result.errors, result.failures)
      out[name] = seen[0].numpy().astype(np.float32)
  finally:
    torch.Tensor.cuda = cuda
  assert set(out) == set(R.EXACT_BITS)
  return out


def cases():
  out = reference_test_images()
  rs = np.random.RandomState(20201007)
  def hw():
    return int(rs.randint(5, 66)), int(rs.randint(5, 66))
  for i in range(6):
    h, w = hw()
    out["rand1_%d_%dx%d" % (i, h, w)] = rs.random_sample((1, h, w)).astype(np.float32)
  for i in range(3):
    h, w = hw()
    out["rand3_%d_%dx%d" % (i, h, w)] = rs.random_sample((3, h, w)).astype(np.float32)
  for i in range(5):
    h, w = hw()
    img = rs.random_sample((h, w)).astype(np.float32)
    if i >= 3:                              # smooth ramps with a little noise: small differences, a peaked histogram
      img = (np.linspace(0.0, 1.0, w, dtype=np.float32)[None, :] * 0.9 + 0.1 * img).astype(np.float32)
    out["rand2d_%d_%dx%d" % (i, h, w)] = img
  for i, shape in enumerate(((1, 17, 33), (3, 9, 21), (23, 41), (64, 65))):
    out["wide%d_%s" % (i, "x".join(str(s) for s in shape))] = (rs.random_sample(shape) * 1.3 - 0.1).astype(np.float32)
  return out


def main():
  check_identities()
  torch.histc = histc_int_as_fp32
  store, gaps = {}, {"gray": {}, "grad": {}}
  names = []
  all_cases = cases()
  for name, img in all_cases.items():
    t = torch.from_numpy(img)
    names.append(name)
    store["img__" + name] = img
    got = {"gray": ref_entropy.grayscale_shannon_entropy(t)}
    if img.ndim == 2:
      got["grad"] = ref_entropy.gradient_shannon_entropy(t)
    want64 = dict(zip(("gray", "grad"), R.scores64(img)))
    for col, h in got.items():
      assert h.dtype == torch.float32
      store[col + "__" + name] = np.float32(h.item())
      if name not in R.EXACT_BITS:
        gaps[col][name] = float(R.ulp_gap(np.float32(h.item()), np.float32(want64[col])))
  store["names"] = np.array(names)
  store["meta"] = np.array("torch %s numpy %s" % (torch.__version__, np.__version__))
  path = os.path.join(HERE, "entropy.npz")
  np.savez_compressed(path, **store)
  print("%s: %d arrays, %.1f KB" % (path, len(store), os.path.getsize(path) / 1e3))
  bound = {
    "what": "fp32 ulps between the REFERENCE's fp32 entropy (torch's fp32 log2 and sum) and float32(the fp64 entropy of the "
            "same integer counts, bins in order), per image; the exact 0-, 1- and 2-bit images are not in it",
    "torch": torch.__version__,
    "per_image": gaps,
    "worst_ulp": {col: max(g.values()) for col, g in gaps.items()},
  }
  with open(os.path.join(HERE, "entropy_bound.json"), "w") as f:
    json.dump(bound, f, indent=1, sort_keys=True)
    f.write("\n")
  print("worst ulp gap:", bound["worst_ulp"])


if __name__ == "__main__":
  main()
