"""Generates tests/golden/lidar_gt.npz by running the REFERENCE's own scripts/export_gt_disp.py.

Run in the build container only (needs /root/reference; the GPU box never has it):

    python tests/golden/make_golden_lidar.py

What it does: imports the reference script by path (setting ``np.int = int`` in THIS process when numpy no longer has it; the
reference file is not touched), writes the synthetic calibration files and .bin scans of tests/lidar_ref.py into a temporary tree of
the shape the script's glob expects (kitti_data_raw/<date>/<drive>/image_0{2,3}/data/*.jpg as empty files), calls its
generate_depth_map for both cameras and both vel_depth values, then its export_gt_disp() on the tree, and stores only the
resulting arrays, the projection matrices it composed, checksums of the inputs and the versions.  The scans are not stored:
lidar_ref.make_scan regenerates them from numpy's frozen legacy generator.  No reference source text is stored in the fixture.

The archive is written with fixed zip timestamps, so a second run gives the same bytes.
"""
import importlib.util
import io
import os
import sys
import tempfile
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = "/root/reference"
sys.path.insert(0, os.path.dirname(HERE))
import lidar_ref as R                                                               # noqa: E402

if not hasattr(np, "int"):
  np.int = int

spec = importlib.util.spec_from_file_location("ref_export_gt_disp", os.path.join(REFERENCE, "scripts", "export_gt_disp.py"))
ref = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ref)


def save_npz(path, store):
  with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
    for key in sorted(store):
      info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
      info.compress_type = zipfile.ZIP_DEFLATED
      info.external_attr = 0o644 << 16
      buf = io.BytesIO()
      np.lib.format.write_array(buf, np.asanyarray(store[key]), allow_pickle=False)
      z.writestr(info, buf.getvalue())


def reference_projection(calib_dir, cam):
  """P_velo2im as generate_depth_map composes it, from the reference's own parser."""
  cam2cam = ref.read_calib_file(os.path.join(calib_dir, "calib_cam_to_cam.txt"))
  velo2cam = ref.read_calib_file(os.path.join(calib_dir, "calib_velo_to_cam.txt"))
  assert isinstance(cam2cam["calib_time"], str) and isinstance(cam2cam["rig"], str)
  velo2cam = np.vstack((np.hstack((velo2cam["R"].reshape(3, 3), velo2cam["T"][..., np.newaxis])), np.array([0, 0, 0, 1.0])))
  rect = np.eye(4)
  rect[:3, :3] = cam2cam["R_rect_00"].reshape(3, 3)
  return np.dot(np.dot(cam2cam["P_rect_0" + str(cam)].reshape(3, 4), rect), velo2cam), cam2cam


def check_general(calib_dir, scan, shape):
  """On the reference alone: no in-bounds point within 1e-9 of a rounding edge, so a last-ulp difference between BLAS and a
  written summation order cannot move a point; and the planted routes are really taken."""
  H, W = shape
  behind = 0
  for cam in (2, 3):
    P, _ = reference_projection(calib_dir, cam)
    velo = scan.copy()
    velo[:, 3] = 1.0
    velo = velo[velo[:, 0] >= 0, :]
    with np.errstate(all="ignore"):
      q = np.dot(P, velo.T).T
      a, b = q[:, 0] / q[:, 2], q[:, 1] / q[:, 2]
      u, v = np.round(a) - 1, np.round(b) - 1
      ok = (u >= 0) & (v >= 0) & (u < W) & (v < H)
    for t in (a[ok], b[ok]):
      edge = np.abs(t - np.floor(t) - 0.5)
      assert edge.min() >= 1e-9, "a point lies %.3e from a half-integer" % edge.min()
    behind += int((q[ok, 2] < 0).sum())
    pix = (v[ok] * W + u[ok]).astype(np.int64)
    assert np.bincount(pix).max() >= 3, "no pixel with several points"
  assert behind >= 4, "only %d in-bounds points with negative q2" % behind
  return behind


def main():
  store = {}
  cwd = os.getcwd()
  with tempfile.TemporaryDirectory() as tmp:
    root = os.path.join(tmp, "kitti_data_raw")
    scans = {}
    for name in sorted(R.SCANS):
      H, W, N, _ = R.SCANS[name]
      date = os.path.join(root, R.DATES[name])
      drive = os.path.join(date, R.DRIVES[name])
      R.write_calibration(date, name)
      for sub in ("image_02", "image_03", "velodyne_points"):
        os.makedirs(os.path.join(drive, sub, "data"))
      for sub in ("image_02", "image_03"):
        open(os.path.join(drive, sub, "data", R.FRAME + ".jpg"), "w").close()
      scan = R.make_scan(name)
      assert scan.shape == (N, 4) and scan.dtype == np.float32
      assert np.signbit(scan[scan[:, 0] == 0, 0]).any() or name == "dyadic"
      velo = os.path.join(drive, "velodyne_points", "data", R.FRAME + ".bin")
      scan.tofile(velo)
      scans[name] = scan
      store["check__scan__" + name] = R.checksum(scan)
      store["shape__" + name] = np.array([H, W], dtype=np.int64)
      if name == "general":
        store["behind__" + name] = np.array(check_general(date, scan, (H, W)), dtype=np.int64)
      for cam in (2, 3):
        P, cam2cam = reference_projection(date, cam)
        store["P%d__%s" % (cam, name)] = P
        store["fx__" + name] = np.array(cam2cam["P_rect_02"].reshape(3, 4)[0, 0], dtype=np.float64)
        for vd in (0, 1):
          with np.errstate(all="ignore"):
            depth = ref.generate_depth_map(date, velo, cam, bool(vd))
          assert depth.shape == (H, W) and depth.dtype == np.float64
          store["depth__%s__cam%d__vd%d" % (name, cam, vd)] = depth
    os.chdir(tmp)
    try:
      with np.errstate(all="ignore"):
        ref.export_gt_disp(root + os.sep)
    finally:
      os.chdir(cwd)
    assert not os.path.exists(os.path.join(tmp, "no_groundtruth.txt"))
    for name in sorted(R.SCANS):
      drive = os.path.join(root, R.DATES[name], R.DRIVES[name])
      bf = 0.54 * store["fx__" + name][()]                            # an np.float64 scalar, as in the reference (a Python float would not promote)
      for cam in (2, 3):
        q = np.load(os.path.join(drive, "disp_0%d" % cam, "data", R.FRAME + ".npy"))
        assert q.dtype == np.uint16 and q.shape == tuple(store["shape__" + name])
        store["export__%s__cam%d" % (name, cam)] = q
        depth = store["depth__%s__cam%d__vd1" % (name, cam)].astype(np.float32)
        with np.errstate(all="ignore"):
          disp = bf / depth
        assert disp.dtype == np.float64, "numpy %s divides a float64 scalar by a float32 array in %s" % (np.__version__, disp.dtype)
        disp[(depth == 0) | (depth > 80)] = 0
        s = 128.0 * disp
        assert s.max() <= 65535
        if name == "general":
          nz = s[s != 0]
          assert np.abs(nz - np.round(nz)).min() >= 1e-9, "a 128 * disp lies within 1e-9 of an integer"
          e80 = np.float32(80)
          assert (depth == np.nextafter(e80, np.float32(np.inf))).any() and (depth == np.nextafter(e80, np.float32(-np.inf))).any()
          assert (depth == e80).any()
  store["meta"] = np.array("numpy %s; float64 scalar / float32 array -> float64" % np.__version__)
  path = os.path.join(HERE, "lidar_gt.npz")
  save_npz(path, store)
  print("%s: %d arrays, %.1f KB" % (path, len(store), os.path.getsize(path) / 1e3))


if __name__ == "__main__":
  main()
