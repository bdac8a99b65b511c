"""Generates tests/golden/visualization.npz by running the REFERENCE's own adaptive_stereo/utils/visualization.py.

Run in the build container only (needs /root/reference and matplotlib; the GPU box has neither):

    python tests/golden/make_golden_visualization.py

That module imports cv2, which is not installed here, for two things: the constant COLOR_RGB2BGR and cvtColor with it.  A stand-in
module of this maker's own (the constant, and a cvtColor that reverses the last axis) is placed in sys.modules first.

What is stored (arrays only, no reference text), per shape of visualization_ref.SHAPES and configuration of CONFIGS:
  check__<case>   checksum of the input, which visualization_ref.make_case regenerates
  u8__<case>      visualize_disp_cv of every image of the batch, stacked: uint8 [B,H,W,3] BGR
  f32__<case>     float32 of visualize_disp_tensorboard's float64, brought to [B,3,H,W]            (where R.stores_float says so)
  rgba__<case>    apply_cmap of the whole batch, float64 [B,H,W,4]                                (where R.stores_float says so)
and table__<map> = the five maps' [259,4] float64 tables read off matplotlib, the three conversions on seeded images, the values
of the (0, 0.6 * 192) range at which a reciprocal lands in another bin (at least one, asserted), and the versions.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REFERENCE = "/root/reference"
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "adaptive-stereo-icra-2021_amd"))
import visualization_ref as R                                                       # noqa: E402
from adaptive_stereo.utils.visualization import colormap_table                      # noqa: E402  (four public calls on a Colormap)

cv2 = types.ModuleType("cv2")
cv2.COLOR_RGB2BGR = 4


def _cvt(im, code):
  assert code == cv2.COLOR_RGB2BGR and im.shape[-1] == 3
  return np.ascontiguousarray(im[..., ::-1])


cv2.cvtColor = _cvt
sys.modules["cv2"] = cv2

import importlib.util                                                               # noqa: E402
import matplotlib                                                                   # noqa: E402
matplotlib.use("Agg")
spec = importlib.util.spec_from_file_location("reference_visualization",
                                              os.path.join(REFERENCE, "adaptive_stereo", "utils", "visualization.py"))
ref = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ref)


def main():
  store = {}
  cmaps = {name: matplotlib.colormaps[name] for name in R.MAPS}
  for name, cm in cmaps.items():
    table, n = colormap_table(cm)
    assert n == 256
    store["table__" + name] = table
  biters = R.reciprocal_biters(0, R.R115)
  assert len(biters) >= 1, "no value found at which the reciprocal form lands in another bin"
  store["reciprocal_biters"] = biters

  for shape in R.SHAPES:
    for config in R.configs_for(shape):
      kind, vmin, vmax, cmap = config
      name = R.case_name(shape, config)
      x = R.make_case(shape, kind)
      t = torch.from_numpy(x)
      store["check__" + name] = R.checksum(x)
      with np.errstate(invalid="ignore", divide="ignore"):
        store["u8__" + name] = np.stack([ref.visualize_disp_cv(t[b], cmap=cmaps[cmap], vmin=vmin, vmax=vmax) for b in range(shape[0])])
        if R.stores_float(shape, config):
          tb = [ref.visualize_disp_tensorboard(t[b], cmap=cmaps[cmap], vmin=vmin, vmax=vmax) for b in range(shape[0])]
          # the reference leaves a map of height 1 or 3 as [H,W,3]
          tb = [a if a.shape == (3, shape[2], shape[3]) and shape[2] not in (1, 3) else np.moveaxis(a, -1, 0) for a in tb]
          store["f32__" + name] = np.stack(tb).astype(np.float32)
          store["rgba__" + name] = ref.apply_cmap(t, vmin=vmin, vmax=vmax, cmap=cmaps[cmap])
  # apply_cmap's own default map (gray) and the raw return shapes of the wrappers on one small case
  x = R.make_case(R.SHAPES[1], "plain")
  store["rgba_default__3x7"] = ref.apply_cmap(torch.from_numpy(x))
  store["tensorboard_raw__3x7"] = ref.visualize_disp_tensorboard(torch.from_numpy(x[0]))
  x = R.make_case(R.SHAPES[2], "plain")
  store["tensorboard_raw__37x53"] = ref.visualize_disp_tensorboard(torch.from_numpy(x[0]), vmin=0, vmax=80).astype(np.float32)
  store["float_image_rgb__37x53"] = ref.float_image_to_cv_uint8(ref.apply_cmap(torch.from_numpy(x[:1]), cmap=cmaps["jet"])[0, :, :, :3],
                                                                encoding="rgb")

  for hw in R.CONVERSION_SHAPES:
    tag = "%dx%d" % hw
    if hw[1] not in (1, 3):                          # (3,H,1) and (3,H,3) already count as channel-last there
      store["cv_rgb__" + tag] = ref.tensor_to_cv_rgb(torch.from_numpy(R.make_image(3, hw)))
    store["cv_rgb_last__" + tag] = ref.tensor_to_cv_rgb(torch.from_numpy(np.ascontiguousarray(np.moveaxis(R.make_image(3, hw), 0, -1))))
    store["cv_gray__" + tag] = ref.tensor_to_cv_gray(torch.from_numpy(R.make_image(1, hw)))
    d = torch.from_numpy(R.make_disp_image(hw))
    store["cv_disp__" + tag] = ref.tensor_to_cv_disp(d)
    store["cv_disp_f32__" + tag] = ref.tensor_to_cv_disp(d, cast_uint8=False)
    store["cv_disp_2d__" + tag] = ref.tensor_to_cv_disp(d[0])
  store["meta"] = np.array("torch %s numpy %s matplotlib %s" % (torch.__version__, np.__version__, matplotlib.__version__))
  path = os.path.join(HERE, "visualization.npz")
  np.savez_compressed(path, **store)
  print("%s: %d arrays, %.1f KB, %d reciprocal biters" % (path, len(store), os.path.getsize(path) / 1e3, len(biters)))


if __name__ == "__main__":
  main()
