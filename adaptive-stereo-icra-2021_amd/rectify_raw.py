"""Rectifies a folder of raw (unrectified) stereo images with a KITTI-style calibration file, on the device
(adaptive_stereo.rectify): what one otherwise does per frame with cv2.initUndistortRectifyMap + cv2.remap on the host.

  python rectify_raw.py --left 2011_09_26/drive_0001_extract/image_02/data --right .../image_03/data \
                        --calib 2011_09_26/calib_cam_to_cam.txt --out rectified [--cams 2 3] [--fill 0]

Pairs are matched by file name.  Writes <out>/left/<name>.png and <out>/right/<name>.png, 8-bit, the rectified value * 255
rounded to the nearest integer (on the device), and prints the rectified intrinsics and the baseline: what
pointcloud.StereoCamera takes.  Pixels of the rectified image that no raw pixel covers carry --fill.
"""
import argparse
import os

import numpy as np
import torch
from PIL import Image

from adaptive_stereo.rectify import KittiRawRectification, Rectifier

EXTENSIONS = (".png", ".jpg", ".jpeg", ".ppm", ".pgm", ".bmp")


def to_u8(img):
  """fp32 [B,3,H,W] in [0, 1] -> uint8 [B,H,W,3] on the device: floor(v * 255 + 0.5), clamped"""
  return (img * 255.0).add_(0.5).floor_().clamp_(0.0, 255.0).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def _load(path, size, channels):
  im = Image.open(path)
  im = im.convert("L" if channels == 1 else "RGB")
  a = np.array(im, dtype=np.uint8)
  if a.shape[:2] != tuple(size):
    raise RuntimeError("%s is %dx%d, the calibration's raw size is %dx%d" % (path, a.shape[0], a.shape[1], size[0], size[1]))
  return np.ascontiguousarray(a.reshape(size[0], size[1], channels))


def rectify_raw(left_dir, right_dir, calib_path, out_dir, cams=(2, 3), fill=0.0, channels=3, device="cuda"):
  """Returns (pairs written, the Rectifier)."""
  calib = KittiRawRectification.from_file(calib_path, cams=cams)
  names = sorted(n for n in os.listdir(left_dir) if n.lower().endswith(EXTENSIONS))
  missing = [n for n in names if not os.path.exists(os.path.join(right_dir, n))]
  if missing:
    raise RuntimeError("%d left images have no right image of the same name in %s (first: %s)" % (len(missing), right_dir, missing[0]))
  rect = Rectifier(calib.view_l, calib.view_r, calib.raw_size, batch=1, channels=channels, fill=fill, device=device)
  cam = rect.camera
  print("Found {} pairs; raw {}x{}, rectified {}x{}".format(len(names), calib.raw_size[0], calib.raw_size[1], rect.H, rect.W))
  print("Rectified intrinsics: fx {:.6f} fy {:.6f} cx {:.6f} cy {:.6f}".format(cam.fx, cam.fy, cam.cx, cam.cy))
  print("Baseline: {:.6f} m".format(cam.baseline))
  print("Valid fraction: left {:.4f} right {:.4f}".format(*rect.valid_fraction()))
  for side in ("left", "right"):
    os.makedirs(os.path.join(out_dir, side), exist_ok=True)
  for ii, name in enumerate(names):
    if ii % 100 == 0:
      print("Finished {}/{} pairs".format(ii, len(names)))
    raw = [torch.from_numpy(_load(os.path.join(d, name), calib.raw_size, channels)[None]).to(rect.device) for d in (left_dir, right_dir)]
    out = [to_u8(t).cpu().numpy()[0] for t in rect(raw[0], raw[1])]              # synchronises
    stem = os.path.splitext(name)[0] + ".png"
    for side, a in zip(("left", "right"), out):
      Image.fromarray(a[:, :, 0] if channels == 1 else a).save(os.path.join(out_dir, side, stem))
  return len(names), rect


if __name__ == "__main__":
  p = argparse.ArgumentParser(description="Rectify raw stereo pairs on the GPU from a KITTI-style calibration file")
  p.add_argument("--left", type=str, required=True, help="folder of the raw left images")
  p.add_argument("--right", type=str, required=True, help="folder of the raw right images (the same file names)")
  p.add_argument("--calib", type=str, required=True, help="calib_cam_to_cam.txt")
  p.add_argument("--out", type=str, required=True)
  p.add_argument("--cams", type=int, nargs=2, default=(2, 3), help="the left and the right camera's number in the file")
  p.add_argument("--fill", type=float, default=0.0, help="value in [0, 1] of rectified pixels outside the raw image")
  p.add_argument("--mono", action="store_true", default=False, help="grey-level cameras (KITTI's 0 and 1)")
  opt = p.parse_args()
  n, _ = rectify_raw(opt.left, opt.right, opt.calib, opt.out, cams=tuple(opt.cams), fill=opt.fill, channels=1 if opt.mono else 3)
  print("Wrote {} rectified pairs to {}".format(n, opt.out))
