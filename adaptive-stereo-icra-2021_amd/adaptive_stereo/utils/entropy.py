"""Shannon entropy of an image's 8-bit intensities and of their horizontal differences, on the device (csrc/entropy.hip).

Reference: adaptive_stereo/utils/entropy.py.  There each function is a chain of torch calls over one image (``.int()``,
``torch.histc``, a masked ``log2``, a sum); here a whole batch is one launch that counts in integers and sums the 256 bins in
fp64 (the arithmetic is a contract: include/adaptive_stereo_hip.h).  A per-image novelty score that needs no network pass:
``ood.precision_recall``, ``ood.ood_threshold`` and ``ood.fcs_histogram`` take either column as they take an FCS column.

  h = grayscale_shannon_entropy(img)                      # 0-d device tensor, no synchronisation
  scores = image_entropy(batch)                           # [B,2]: column 0 intensities, column 1 horizontal differences
  collector = EntropyCollector(1000); collector.add(batch); collector.scores()
"""
import torch

from .. import _native as nat
from ..collect import RowCursor, check_f32

__all__ = ["grayscale_shannon_entropy", "gradient_shannon_entropy", "image_entropy", "EntropyCollector", "release_workspaces"]

_WORKSPACES = {}     # (device index, stream) -> zeroed workspace; the kernel hands it back zeroed, so it is cleared once


def release_workspaces():
  """Drops the workspaces that image_entropy and the two reference-named functions keep per device and stream; the next call
  on a stream makes a fresh, zeroed one.  Call it after a launch that failed or was abandoned part-way (its workspace may not
  be all zero any more), or to give the memory back once the streams are gone."""
  _WORKSPACES.clear()


def _workspace_bytes(B):
  n = int(nat.load().as_image_entropy_workspace(int(B)))
  if n <= 0:
    raise RuntimeError("adaptive_stereo.utils.entropy: a batch of %d images is outside the kernel's range [1, 65535]" % B)
  return n


def _workspace(device, B):
  key = (device.index, torch.cuda.current_stream(device).cuda_stream)
  need = _workspace_bytes(B)
  ws = _WORKSPACES.get(key)
  if ws is None or ws.numel() < need:
    if torch.cuda.is_current_stream_capturing():      # it would come from the graph's pool and outlive the graph in this cache
      raise RuntimeError("adaptive_stereo.utils.entropy: the first call on a stream (or the first with a batch this large) "
                         "sizes its workspace; make it once outside the capture, or capture EntropyCollector.add")
    ws = _WORKSPACES[key] = torch.zeros(need, dtype=torch.uint8, device=device)
  return ws


def _as_batch(images, what):
  """A contiguous fp32 [B,C,H,W] view (or copy) of [B,C,H,W] / [B,H,W]."""
  nat.require_gpu(images)
  x = nat.f32c(images.detach())
  if x.dim() == 3:
    x = x[:, None]
  if x.dim() != 4 or x.numel() == 0:
    raise RuntimeError("adaptive_stereo.utils.entropy: %s has shape %s, expected [B,C,H,W] or [B,H,W]" % (what, tuple(images.shape)))
  return x


def _launch(x, scores, capacity, cursor, dropped, hist, workspace):
  B, C, H, W = x.shape
  with torch.cuda.device(x.device):
    nat.call("as_image_entropy", nat.ptr(x), B, C, H, W, nat.ptr(scores), capacity, nat.ptr(cursor), nat.ptr(dropped),
             nat.ptr(hist), nat.ptr(workspace), nat.stream())


def image_entropy(images, hist=False):
  """scores [B,2] of [B,C,H,W] or [B,H,W] images with values in [0, 1]: per image the entropy in bits of the 256-bin histogram
  of int(255 * x) over all its C planes (column 0) and of the horizontal differences of those integers inside each row
  (column 1), both normalised by the plane's size as the reference normalises.  hist=True: (scores, counts int32 [B,2,256]).
  Never synchronises."""
  with torch.no_grad():
    x = _as_batch(images, "images")
    B = x.shape[0]
    scores = torch.empty(B, 2, dtype=torch.float32, device=x.device)
    counts = torch.empty(B, 2, 256, dtype=torch.int32, device=x.device) if hist else None
    with torch.cuda.device(x.device):
      ws = _workspace(x.device, B)
    _launch(x, scores, B, None, None, counts, ws)
  return (scores, counts) if hist else scores


def _single(img, what):
  nat.require_gpu(img)
  if img.dim() < 2:
    raise RuntimeError("adaptive_stereo.utils.entropy: %s needs a [..., H, W] image (got shape %s)" % (what, tuple(img.shape)))
  H, W = img.shape[-2], img.shape[-1]
  return image_entropy(img.reshape(1, -1, H, W))[0]


def grayscale_shannon_entropy(img):
  """The entropy in bits of the intensity distribution of ONE image [..., H, W] with values in [0, 1]; every leading dimension
  is counted into the same histogram and the normaliser is H * W, as in the reference.  A 0-d device tensor."""
  return _single(img, "grayscale_shannon_entropy")[0]


def gradient_shannon_entropy(img):
  """The entropy in bits of the horizontal differences of ONE [H, W] image's 8-bit intensities.  A 0-d device tensor; NaN for
  W == 1 (no differences)."""
  assert len(img.shape) == 2
  return _single(img, "gradient_shannon_entropy")[1]


class EntropyCollector(RowCursor):
  """A [capacity,2] score buffer on the device with its cursor and a counter of the rows that did not fit, allocated once:
  ood.FcsCollector for image_entropy's two columns."""

  def __init__(self, capacity, device="cuda"):
    super().__init__("EntropyCollector", capacity, device)
    self._scores = torch.zeros(self.capacity, 2, dtype=torch.float32, device=self.device)
    self._workspace = None                                               # sized by the first add()

  def add(self, images):
    """Appends the B rows of a contiguous fp32 batch [B,C,H,W] or [B,H,W] at the cursor.  After the first call (which sizes the
    workspace) it allocates nothing and never synchronises; inside a captured graph every replay appends.  Rows beyond the
    capacity are counted in dropped()."""
    check_f32("EntropyCollector.add", "images", images, ((3, 4), "[B,C,H,W] or [B,H,W]"), self._scores.device)
    if images.numel() == 0:
      raise RuntimeError("EntropyCollector.add: images is empty (shape %s)" % (tuple(images.shape),))
    x = images if images.dim() == 4 else images[:, None]
    need = _workspace_bytes(x.shape[0])
    if self._workspace is None or self._workspace.numel() < need:
      if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("EntropyCollector.add: the first add() of a batch this large sizes the workspace; call it once "
                           "outside the capture")
      self._workspace = torch.zeros(need, dtype=torch.uint8, device=self.device)
    _launch(x, self._scores, self.capacity, self._cursor, self._dropped, None, self._workspace)

  def scores(self):
    """Synchronises.  The rows in use, [n,2] (a clone: later add() calls do not change it)."""
    return self._scores[:self.rows_in_use()].clone()
