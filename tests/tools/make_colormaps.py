"""Writes adaptive_stereo/utils/colormaps.json from the matplotlib installed on the build machine.

    python tests/tools/make_colormaps.py

Per map the reference names (magma, inferno, hot, jet, gray) a float64 [N + 3, 4] RGBA table: the N = 256 entries, then the
colours matplotlib gives to values below the range, above it, and to NaN.  Only public calls are used, the same four that
adaptive_stereo.utils.visualization.colormap_table makes on any colour-map object, so the package never imports matplotlib.
The file is text (json writes a float's shortest repr, which reads back to the same float64: the round trip is asserted).
The data is matplotlib's; its version is recorded beside it.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "adaptive-stereo-icra-2021_amd"))

NAMES = ("magma", "inferno", "hot", "jet", "gray")


def main():
  import matplotlib
  from adaptive_stereo.utils.visualization import colormap_table, COLORMAPS_PATH
  store = {}
  for name in NAMES:
    table, n = colormap_table(matplotlib.colormaps[name])
    assert table.shape == (259, 4) and n == 256 and table.dtype == np.float64
    store[name] = table.tolist()
  with open(COLORMAPS_PATH, "w") as f:
    json.dump({"matplotlib_version": matplotlib.__version__, "tables": store}, f, separators=(",", ":"))
    f.write("\n")
  with open(COLORMAPS_PATH, "r") as f:
    back = json.load(f)["tables"]
  for name in NAMES:
    assert np.array_equal(np.array(back[name], dtype=np.float64), colormap_table(matplotlib.colormaps[name])[0]), name
  print("%s: %s, matplotlib %s, %.1f KB" % (COLORMAPS_PATH, ", ".join(NAMES), matplotlib.__version__,
                                             os.path.getsize(COLORMAPS_PATH) / 1e3))


if __name__ == "__main__":
  main()
