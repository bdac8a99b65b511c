"""Ground-truth disparity for KITTI raw from its Velodyne scans: the counterpart of the reference's scripts/export_gt_disp.py,
with the projection, the nearest return per pixel and the conversion to uint16 = 128 * disp on the device (adaptive_stereo.lidar).

  python export_gt_disp.py --dataset_path /data/kitti_data_raw [--batch 8] [--no_cleanup]

The same tree walk (*/*/image_02/*/*.jpg, the scan beside it under velodyne_points, the calibration of the date folder), the same
disp_02/ and disp_03/ .npy files beside image_02 (uint16, the image's shape: what utils/dataset_utils.raw_disp_kitti_raw reads at
1/128) and the same ./no_groundtruth.txt for frames without a scan.  No jpg is ever decoded.  Two differences, both in
INTEGRATION.md §E: the nearest return is chosen per pixel (the reference merges pixel (r, W-1) with (r+1, 0)), and a disparity
that does not fit uint16 is written as 0 and reported, where the reference stops at an assertion.
"""
import argparse
import glob
import os

import numpy as np
import torch

from adaptive_stereo.lidar import KittiCalibration, LidarGroundTruth, load_velodyne_bin


def _flush(gt, frames, cleanup_old):
  """frames: [(image path, scan)] of one date folder, at most gt.B of them."""
  points, counts = gt.upload([s for _, s in frames])
  overflow = 0
  for cam in (2, 3):
    frame = gt.project(points, counts, cam=cam, vel_depth=True, quantize=True)
    disp = frame.disp_u16.cpu().numpy()                       # synchronises
    overflow += int(frame.overflow.sum())
    for b, (im, _) in enumerate(frames):
      disp_path = im.replace("image_02", "disp_0%d" % cam).replace(".jpg", ".npy")
      disp_folder = os.path.abspath(os.path.join(disp_path, ".."))
      if cleanup_old:                                         # files an older export left one level up, beside data/ (the parent
        stale = glob.glob(os.path.join(os.path.dirname(disp_folder), "*.npy"))      # is named outright: data/ may not exist yet)
        if stale:
          print("Found {} existing files not in data/, deleting".format(len(stale)))
          for f in stale:
            os.remove(f)
      os.makedirs(disp_folder, exist_ok=True)
      np.save(disp_path, disp[b])
  if overflow:
    print("WARNING: {} pixels had a disparity above 65535 / 128 and were written as 0".format(overflow))
  return overflow


def export_gt_disp(dataset_path, cleanup_old=True, batch=8, device="cuda"):
  """Creates disp_02/ and disp_03/ beside image_02/ for every frame with a scan.  Returns (frames written, frames skipped)."""
  imgs_left = sorted(glob.glob(os.path.join(dataset_path, "*/*/image_02/*/*.jpg")))
  imgs_right = glob.glob(os.path.join(dataset_path, "*/*/image_03/*/*.jpg"))
  print("Found {} left images and {} right images".format(len(imgs_left), len(imgs_right)))
  assert len(imgs_left) == len(imgs_right)

  written = skipped = 0
  engines = {}                                                # one set of buffers per date folder (its calibration and image size)
  pending, pending_dir = [], None
  for ii, im in enumerate(imgs_left):
    if ii % 100 == 0:
      print("Finished {}/{} images".format(ii, len(imgs_left)))
    velo = im.replace("image_02", "velodyne_points").replace(".jpg", ".bin")
    if not os.path.exists(velo):
      with open("./no_groundtruth.txt", "a") as f:
        print("WARNING: Had to skip {} because no velodyne file was found".format(im))
        f.write(im + "\n")
      skipped += 1
      continue
    calib_dir = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(im))))      # <date>/<drive>/image_02/data/x.jpg
    if pending and (calib_dir != pending_dir or len(pending) == batch):
      _flush(engines[pending_dir], pending, cleanup_old)
      written += len(pending)
      pending = []
    if calib_dir not in engines:
      engines[calib_dir] = LidarGroundTruth(KittiCalibration.from_files(calib_dir), batch=batch, device=device)
    scan = load_velodyne_bin(velo)
    if scan.shape[0] > engines[calib_dir].max_points:
      raise RuntimeError("%s holds %d points, more than max_points = %d" % (velo, scan.shape[0], engines[calib_dir].max_points))
    pending.append((im, scan))
    pending_dir = calib_dir
  if pending:
    _flush(engines[pending_dir], pending, cleanup_old)
    written += len(pending)
  torch.cuda.synchronize()
  return written, skipped


if __name__ == "__main__":
  p = argparse.ArgumentParser(description="Export KITTI raw ground-truth disparity from Velodyne scans on the GPU")
  p.add_argument("--dataset_path", type=str, required=True)
  p.add_argument("--no_cleanup", action="store_true", default=False, help="keep .npy files an older export left beside data/")
  p.add_argument("--batch", type=int, default=8, help="frames per launch")
  opt = p.parse_args()
  n, k = export_gt_disp(opt.dataset_path, cleanup_old=not opt.no_cleanup, batch=opt.batch)
  print("Wrote disparity for {} frames, skipped {}".format(n, k))
