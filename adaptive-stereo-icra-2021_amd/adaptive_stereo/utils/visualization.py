"""Colour-mapped disparity and error images, on the device (csrc/visualize.hip).

The reference's utils/visualization.py copies the map to the host, normalises it there and pushes every pixel through matplotlib's
Colormap.__call__.  Here one or two launches write the finished image; the arithmetic is fixed op by op in
include/adaptive_stereo_hip.h and reproduces the reference bit for bit (tests/golden/visualization.npz).

Per frame, for a ROS node or a video writer:

  painter = DisparityPainter(height, width, batch=1, cmap="magma", vmin=0, vmax=0.6 * 192, order="bgr")   # allocates everything
  image = painter.paint(disp)                # [B,H,W,3] uint8 on the device; no allocation, no synchronisation, graph-capturable
  error = painter.paint_error(pred, gt)      # |gt - pred| formed on the fly
  left = painter.rgb(color)                  # [B,3,H,W] float in [0,1] -> [B,H,W,3] uint8
The views a call returns alias the painter's buffers: the next call of the same kind overwrites them.

The reference's own names (apply_cmap, visualize_disp_cv, visualize_disp_tensorboard, tensor_to_cv_rgb / _gray / _disp,
float_image_to_cv_uint8, maybe_put_channel_dim_first / _last) are here with its call shapes and return numpy arrays of its shapes
and dtypes, computed by the same kernels with one device-to-host copy of the result.  Its callers hand them .cpu() tensors, so
this module — the one exception to "the product refuses CPU tensors" — uploads a CPU tensor: there is one arithmetic.
Two documented differences: visualize_disp_tensorboard returns float32 (the table rounded once), not float64; a value whose
255-fold lies outside 0 .. 255 saturates in the uint8 conversions, where the reference's astype(np.uint8) is unspecified.

cmap= takes a name of a packaged table (magma, inferno, hot, jet, gray: matplotlib's data, written by
tests/tools/make_colormaps.py), None (gray for apply_cmap, magma elsewhere, as in the reference) or any object that behaves like
a matplotlib Colormap.  Neither matplotlib nor cv2 is imported.
"""
import json
import os

import numpy as np
import torch

from .. import _native as nat

COLORMAPS_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "colormaps.json")
MODES = {"u8_rgb": 0, "u8_bgr": 1, "f32": 2, "index": 3}
MAX_N = 256

_packaged = None


def colormap_table(cmap):
  """(float64 [N + 3, 4] RGBA table, N) of a matplotlib-like colour map: its N entries, then the colours it gives to a value
  below the range, above it, and to NaN.  Public calls only."""
  n = int(cmap.N)
  if not 1 <= n <= MAX_N:
    raise ValueError("colormap_table: the colour map has N = %d entries, outside [1, %d]" % (n, MAX_N))
  body = np.asarray(cmap(np.arange(n)), dtype=np.float64).reshape(n, 4)
  tail = [np.asarray(cmap(v), dtype=np.float64).reshape(4) for v in (-1.0, 2.0, float("nan"))]
  return np.ascontiguousarray(np.concatenate([body, np.stack(tail)], axis=0)), n


def packaged_colormaps():
  """{name: float64 [259, 4]} of the packaged tables."""
  global _packaged
  if _packaged is None:
    with open(COLORMAPS_PATH, "r") as f:                   # text: a float's shortest repr reads back to the same float64
      _packaged = {k: np.array(v, dtype=np.float64).reshape(-1, 4) for k, v in json.load(f)["tables"].items()}
  return _packaged


def resolve_colormap(cmap, default="magma"):
  """(float64 [N + 3, 4], N) for a name, None (-> default) or a colour-map object."""
  if cmap is None:
    cmap = default
  if isinstance(cmap, str):
    tables = packaged_colormaps()
    if cmap not in tables:
      raise ValueError("unknown colour map %r (packaged: %s); pass a Colormap object for any other" % (cmap, ", ".join(sorted(tables))))
    return tables[cmap], tables[cmap].shape[0] - 3
  return colormap_table(cmap)


def table_u8(table):
  """uint8 [N + 3, 4]: (255.0 * rgb).astype(uint8), the reference's float_image_to_cv_uint8 applied to the table once."""
  out = np.zeros((table.shape[0], 4), np.uint8)
  out[:, :3] = (255.0 * table[:, :3]).astype(np.uint8)
  return out


_device_tables = {}


def _device_table(cmap, table, kind, device):
  """The table as the kernels read it (kind "u8": uint8 [N+3,4]; "f32": fp32 [N+3,4]) on `device`.  A packaged map is uploaded
  once per device and kind; the table of a colour-map object is uploaded for the painter that asked."""
  key = (cmap, kind, str(device)) if isinstance(cmap, str) else None
  if key is not None and key in _device_tables:
    return _device_tables[key]
  host = table_u8(table) if kind == "u8" else table.astype(np.float32)
  dev = torch.from_numpy(np.ascontiguousarray(host)).to(device)
  if key is not None:
    _device_tables[key] = dev
  return dev


def _device(device=None):
  dev = torch.device("cuda" if device is None else device)
  if dev.type != "cuda":
    raise RuntimeError("adaptive_stereo: the colour-mapping kernels live on the GPU (got %s)" % dev)
  return torch.device("cuda", torch.cuda.current_device()) if dev.index is None else dev


def _upload(t, device=None):
  """fp32 contiguous device tensor of a CPU or device tensor (or numpy array)."""
  if isinstance(t, np.ndarray):
    t = torch.from_numpy(t)
  if not torch.is_tensor(t):
    raise TypeError("expected a tensor, got %s" % type(t).__name__)
  t = t.detach()
  if not t.is_cuda:
    t = t.to(_device(device))
  return t.float().contiguous()


def _bounds(vmin, vmax):
  """(automatic, lo, hi, den) as as_colormap_apply takes them.  Both fixed: den is the difference of the two Python floats,
  rounded once."""
  automatic = (1 if vmin is None else 0) | (2 if vmax is None else 0)
  lo = 0.0 if vmin is None else float(np.float32(float(vmin)))
  hi = 0.0 if vmax is None else float(np.float32(float(vmax)))
  den = float(np.float32(float(vmax) - float(vmin))) if automatic == 0 else 0.0
  return automatic, lo, hi, den


def colormap_launch(x, y, shape, bounds, workspace, table, n, mode, out):
  """as_colormap_range (only with an automatic bound) + as_colormap_apply on the current stream of x's device."""
  B, H, W = shape
  automatic, lo, hi, den = bounds
  with torch.cuda.device(x.device):
    if automatic:
      nat.call("as_colormap_range", nat.ptr(x), nat.ptr(y), B, H, W, nat.ptr(workspace), nat.stream())
    nat.call("as_colormap_apply", nat.ptr(x), nat.ptr(y), B, H, W, automatic, lo, hi, den,
             nat.ptr(workspace) if automatic else None, nat.ptr(table), n, mode, nat.ptr(out), nat.stream())


def _workspace(B, HW, device):
  ws = nat.load().as_colormap_workspace(B, HW)
  if ws < 0:
    raise ValueError("a batch of %d maps of %d pixels is outside what the kernels index" % (B, HW))
  return torch.empty(ws // 4, dtype=torch.float32, device=device)


class DisparityPainter(object):
  """[B,1,H,W] fp32 -> colour images, with every buffer allocated here.  out: "u8" ([B,H,W,3] uint8 in `order`), "f32"
  ([B,3,H,W] fp32, RGB planes) or "index" ([B,H,W] int16 table index; N, N+1, N+2 = under, over, bad).  vmin / vmax: a number
  fixes the bound, None takes it from each image."""

  def __init__(self, height, width, batch=1, cmap="magma", vmin=None, vmax=None, order="bgr", out="u8", device=None):
    self.H, self.W, self.B = int(height), int(width), int(batch)
    if self.H < 1 or self.W < 1 or self.B < 1:
      raise ValueError("DisparityPainter: height %d, width %d and batch %d must be positive" % (self.H, self.W, self.B))
    if order not in ("rgb", "bgr") or out not in ("u8", "f32", "index"):
      raise ValueError("DisparityPainter: order %r (rgb or bgr), out %r (u8, f32 or index)" % (order, out))
    self.order, self.out = order, out
    self.device = dev = _device(device)
    cmap = "magma" if cmap is None else cmap
    self.table, self.N = resolve_colormap(cmap)
    self.bounds = _bounds(vmin, vmax)
    B, H, W = self.B, self.H, self.W
    self._ws = _workspace(B, H * W, dev)
    if out == "u8":
      self.mode = MODES["u8_" + order]
      self._table = _device_table(cmap, self.table, "u8", dev)
      self._out = torch.empty(B, H, W, 3, dtype=torch.uint8, device=dev)
    elif out == "f32":
      self.mode = MODES["f32"]
      self._table = _device_table(cmap, self.table, "f32", dev)
      self._out = torch.empty(B, 3, H, W, dtype=torch.float32, device=dev)
    else:
      self.mode = MODES["index"]
      self._table = None
      self._out = torch.empty(B, H, W, dtype=torch.int16, device=dev)
    self._rgb = torch.empty(B, H, W, 3, dtype=torch.uint8, device=dev)

  def _check(self, name, t, channels=1):
    if not torch.is_tensor(t) or not t.is_cuda or t.device != self.device:
      raise RuntimeError("DisparityPainter: %s must be a tensor on %s (got %s); the reference-named functions of this module "
                         "upload CPU tensors" % (name, self.device, t.device if torch.is_tensor(t) else type(t).__name__))
    if t.dtype != torch.float32 or not t.is_contiguous():
      raise RuntimeError("DisparityPainter: %s must be contiguous fp32 (got %s, contiguous=%s)" % (name, t.dtype, t.is_contiguous()))
    shape = tuple(t.shape)
    if t.dim() == 2:
      shape = (1, channels) + shape if channels == 1 else shape
    elif t.dim() == 3:
      shape = ((shape[0], 1) + shape[1:]) if channels == 1 else (1,) + shape
    if len(shape) != 4 or shape[1] != channels or shape[2:] != (self.H, self.W) or not 1 <= shape[0] <= self.B:
      raise RuntimeError("DisparityPainter: %s has shape %s, expected [b <= %d, %d, %d, %d]"
                         % (name, tuple(t.shape), self.B, channels, self.H, self.W))
    return shape[0]

  def _paint(self, x, y, b):
    colormap_launch(x, y, (b, self.H, self.W), self.bounds, self._ws, self._table, self.N, self.mode, self._out)
    return self._out[:b]

  def paint(self, disp):
    """disp [b,1,H,W] (or [b,H,W], [H,W]) fp32 on the device -> a view of the first b images of the output buffer."""
    return self._paint(disp, None, self._check("disp", disp))

  def paint_error(self, pred, gt):
    """The colour map of |gt - pred|, never materialised."""
    b = self._check("pred", pred)
    if self._check("gt", gt) != b:
      raise RuntimeError("DisparityPainter: pred and gt hold different numbers of images")
    return self._paint(pred, gt, b)

  def rgb(self, img):
    """img [b,3,H,W] (or [3,H,W]) fp32 in [0,1] -> [b,H,W,3] uint8 = trunc(255 * v) in this painter's channel order."""
    b = self._check("img", img, channels=3)
    with torch.cuda.device(self.device):
      nat.call("as_image_to_cv", nat.ptr(img), b, 3, self.H, self.W, 1 if self.order == "bgr" else 0, 0.0, 0, nat.ptr(self._rgb),
               nat.stream())
    return self._rgb[:b]


def colormap(value, cmap="magma", vmin=None, vmax=None, out="u8", order="bgr", error_to=None):
  """One-off functional form: value [B,1,H,W] (CPU or device) -> a new device tensor in the layout of DisparityPainter's `out`.
  error_to: paint |error_to - value| instead.  Allocates the output and the workspace (a packaged table is uploaded once per
  device and reused); a per-frame caller keeps a DisparityPainter."""
  x = _upload(value)
  if x.dim() != 4 or x.shape[1] != 1:
    raise ValueError("colormap: value has shape %s, expected [B,1,H,W]" % (tuple(value.shape),))
  y = None if error_to is None else _upload(error_to, x.device)
  if y is not None and y.shape != x.shape:
    raise ValueError("colormap: error_to has shape %s, value %s" % (tuple(y.shape), tuple(x.shape)))
  painter = DisparityPainter(x.shape[2], x.shape[3], batch=x.shape[0], cmap=cmap, vmin=vmin, vmax=vmax, order=order, out=out,
                             device=x.device)
  return painter._paint(x, y, x.shape[0])


# ---- the reference's names ----------------------------------------------------------------------------------------------------
def _channel_count_ok(n):
  return n in (1, 3)


def maybe_put_channel_dim_first(x):
  """[H,W,C] -> [C,H,W]; an array whose first axis already has length 1 or 3 is returned as it is."""
  return x if _channel_count_ok(x.shape[0]) else np.moveaxis(x, -1, 0)


def maybe_put_channel_dim_last(x):
  """[C,H,W] -> [H,W,C]; an array whose last axis already has length 1 or 3 is returned as it is."""
  return x if _channel_count_ok(x.shape[-1]) else np.moveaxis(x, 0, -1)


def _scale255(t, div=0.0, as_float=False):
  """255.0f * v (then / div) element by element on the device, in t's own shape -> numpy uint8 (or float32)."""
  x = _upload(t)
  n = x.numel()
  if n == 0:
    raise ValueError("empty image")
  out = torch.empty(x.shape, dtype=torch.float32 if as_float else torch.uint8, device=x.device)
  with torch.cuda.device(x.device):
    nat.call("as_image_to_cv", nat.ptr(x), 1, 1, 1, n, 0, float(div), 1 if as_float else 0, nat.ptr(out), nat.stream())
  return out.cpu().numpy()


def tensor_to_cv_disp(disp_t, cast_uint8=True):
  """disp_t (1,H,W), (H,W,1) or (H,W) -> [H,W,1] = trunc(255 * d / W), uint8, or float32 when not cast_uint8."""
  if len(disp_t.shape) == 2:
    disp_t = disp_t.unsqueeze(-1)
  shape = tuple(disp_t.shape)
  moved = not _channel_count_ok(shape[-1])                           # maybe_put_channel_dim_last moves axis 0 to the end
  width = shape[2] if moved else shape[1]
  out = _scale255(disp_t, div=float(width), as_float=not cast_uint8)
  return np.moveaxis(out, 0, -1) if moved else out


def tensor_to_cv_rgb(rgb_t):
  """rgb_t (3,H,W) or (H,W,3), values in [0,1] -> [H,W,3] uint8 BGR."""
  assert len(rgb_t.shape) == 3
  shape = tuple(rgb_t.shape)
  if _channel_count_ok(shape[-1]):                                   # already channel-last as the reference sees it
    assert shape[-1] == 3, "tensor_to_cv_rgb: three channels expected"
    return np.ascontiguousarray(_scale255(rgb_t)[..., ::-1])
  assert shape[0] == 3, "tensor_to_cv_rgb: three channels expected"
  x = _upload(rgb_t)
  out = torch.empty(shape[1], shape[2], 3, dtype=torch.uint8, device=x.device)
  with torch.cuda.device(x.device):
    nat.call("as_image_to_cv", nat.ptr(x), 1, 3, shape[1], shape[2], 1, 0.0, 0, nat.ptr(out), nat.stream())
  return out.cpu().numpy()


def tensor_to_cv_gray(gray_t):
  """gray_t (1,H,W) or (H,W,1), values in [0,1] -> [H,W,1] uint8."""
  assert len(gray_t.shape) == 3
  return maybe_put_channel_dim_last(_scale255(gray_t))


def _as_b1hw(disp_t, who):
  shape = tuple(disp_t.shape)
  if len(shape) == 2:
    disp_t = disp_t.reshape((1, 1) + shape)
  elif len(shape) == 3:
    disp_t = disp_t.unsqueeze(0)
  if len(disp_t.shape) != 4 or disp_t.shape[1] != 1:
    raise ValueError("%s: shape %s, expected (1,H,W), (H,W) or (B,1,H,W)" % (who, shape))
  return disp_t


def apply_cmap(value, vmin=None, vmax=None, cmap=None):
  """value [B,1,H,W] -> float64 RGBA [B,H,W,4], normalised per image where a bound is None.  cmap None: gray."""
  assert len(value.shape) == 4
  x = _upload(value)
  if x.shape[1] != 1:
    raise ValueError("apply_cmap: value has shape %s, expected [B,1,H,W]" % (tuple(value.shape),))
  painter = DisparityPainter(x.shape[2], x.shape[3], batch=x.shape[0], cmap="gray" if cmap is None else cmap, vmin=vmin, vmax=vmax,
                             out="index", device=x.device)
  return painter.table[painter.paint(x).cpu().numpy().astype(np.int64)]


def visualize_disp_tensorboard(disp_t, cmap=None, vmin=None, vmax=None):
  """A disparity image (1,H,W) for tensorboard's add_image: [3,H,W] RGB in [0,1] — float32 here, float64 in the reference.
  As there, a map of height 1 or 3 comes back as [H,W,3]."""
  x = _as_b1hw(disp_t, "visualize_disp_tensorboard")
  out = colormap(x[:1], cmap=cmap, vmin=vmin, vmax=vmax, out="f32")[0].cpu().numpy()
  return out if out.shape[1] not in (1, 3) else np.moveaxis(out, 0, -1)


def visualize_disp_cv(disp_t, cmap=None, vmin=None, vmax=None):
  """A disparity image (1,H,W) or (H,W) -> [H,W,3] uint8 BGR, what cv.imshow / cv.imwrite / cv2_to_imgmsg("bgr8") take."""
  x = _as_b1hw(disp_t, "visualize_disp_cv")
  return colormap(x[:1], cmap=cmap, vmin=vmin, vmax=vmax, out="u8", order="bgr")[0].cpu().numpy()


def float_image_to_cv_uint8(float_im, encoding="rgb"):
  """A host float image [H,W,3] in [0,1] -> uint8 = trunc(255 x), red and blue swapped when encoding is "rgb".  The input is a
  numpy array (float64 from apply_cmap), which fp32 kernels cannot reproduce, so this one stays on the host."""
  image = np.asarray(float_im)
  if image.ndim != 3:
    raise ValueError("float_image_to_cv_uint8: an [H,W,C] image is expected, got shape %s" % (image.shape,))
  low, high = image.min(), image.max()
  if not (low >= 0 and high <= 1):
    print("float_image_to_cv_uint8: values span [%g, %g], outside [0, 1]; the uint8 cast is unspecified there" % (low, high))
  scaled = (image * 255.0).astype(np.uint8)
  if encoding != "rgb":
    return scaled
  return np.ascontiguousarray(np.flip(scaled, axis=-1))
