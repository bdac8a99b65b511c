"""What the device-side collectors share: the row cursor of ood.FcsCollector, utils.entropy.EntropyCollector and
cv_probe.CostVolumeProbe; the check of a tensor handed to a kernel as it is, which confidence.SparsificationCollector uses too;
and the eval-mode pass over a dataset that feeds them."""
import torch


def check_f32(who, name, t, dims=None, device=None, numel=None):
  """Refuses what a kernel cannot read in place: `t` must be a contiguous fp32 GPU tensor, of a rank in dims[0] (dims is
  (ranks, label), e.g. ((4,), "[B,D,H,W]")), on `device` and of `numel` elements, each where given."""
  if not isinstance(t, torch.Tensor) or not t.is_cuda:
    raise RuntimeError("adaptive_stereo: tensors must live on the GPU (got %s for %s); there is no CPU path"
                       % (getattr(t, "device", type(t)), name))
  ranks, label = dims if dims is not None else (None, "")
  if t.dtype != torch.float32 or not t.is_contiguous() or (ranks is not None and t.dim() not in ranks) or \
     (device is not None and t.device != device) or (numel is not None and t.numel() != numel):
    raise RuntimeError("%s: expected a contiguous fp32 %stensor%s on %s for %s (got %s, %s, %s, contiguous=%s)"
                       % (who, label + " " if label else "", "" if numel is None else " of %d elements" % numel,
                          "the GPU" if device is None else device, name, tuple(t.shape), t.dtype, t.device, t.is_contiguous()))


def check_shape(who, name, t, shape, device):
  """After check_f32: `t` has exactly `shape` and lives on `device`."""
  if tuple(t.shape) != tuple(shape) or t.device != device:
    raise RuntimeError("%s: %s must be %s on %s (got %s on %s)" % (who, name, tuple(shape), device, tuple(t.shape), t.device))


def check_u8(who, name, t, shape, device):
  """Refuses what is not a contiguous uint8 tensor of exactly `shape` on `device`."""
  if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or not t.is_contiguous() or tuple(t.shape) != tuple(shape) or \
     t.device != device:
    raise RuntimeError("%s: %s must be a contiguous uint8 %s tensor on %s (got %s, %s, %s)"
                       % (who, name, tuple(shape), device, tuple(getattr(t, "shape", ())), getattr(t, "dtype", None),
                          getattr(t, "device", None)))


def gpu_device(who, device):
  """torch.device(device), refused unless it is a GPU: what holds device buffers has no CPU path."""
  dev = torch.device(device)
  if dev.type != "cuda":
    raise RuntimeError("adaptive_stereo: %s lives on the GPU (got %s); there is no CPU path" % (who, dev))
  return dev


def int_in(who, name, value, lo, hi):
  v = int(value)
  if v != value or not lo <= v <= hi:
    raise ValueError("%s: %s %r must be an integer in %d .. %d" % (who, name, value, lo, hi))
  return v


class MapOperator(object):
  """What the operators on maps [batch,1,height,width] with buffers fixed at construction share (LeftRightConsistency,
  DisparityFilter, SemiGlobalMatcher, DisparitySmoother): the size, the device, the check of an argument against them and the shares of the codes."""

  def __init__(self, height, width, batch, device):
    who = type(self).__name__
    self.H, self.W, self.B = int(height), int(width), int(batch)
    if self.H < 1 or self.W < 1 or self.B < 1:
      raise ValueError("%s: size %r x %r, batch %r" % (who, height, width, batch))
    self.device = gpu_device(who, device)

  def _zeros(self, shape, dtype):
    t = torch.zeros(shape, dtype=dtype, device=self.device)
    self._buffers_on = t.device                              # with the index that `device` may lack
    return t

  def buffers_device(self):
    """The device the buffers live on, with the index that the ``device`` argument may lack."""
    return self._buffers_on

  def _check_map(self, who, name, t, channels=1):
    check_f32(who, name, t, ((4,), "[B,%s,H,W]" % ("1" if channels == 1 else "C")))
    check_shape(who, name, t, (self.B, channels, self.H, self.W), self._buffers_on)

  def _fractions(self, counts):
    """Synchronises.  numpy fp64: int32 counts of pixels as shares of an image."""
    return counts.cpu().numpy().astype("float64") / float(self.H * self.W)


class RowCursor(object):
  """The device-side state of a collector of `capacity` rows: the cursor its kernel appends at and a counter of the rows that did
  not fit (as_cursor_advance_enqueue keeps both), allocated once.  A subclass adds its row buffers, add() and its accessor."""

  def __init__(self, who, capacity, device):
    self.capacity = int(capacity)
    if self.capacity < 1:
      raise ValueError("%s: capacity %r must be at least 1" % (who, capacity))
    self.device = gpu_device(who, device)
    self._state = torch.zeros(2, dtype=torch.int32, device=self.device)  # cursor, dropped
    self._cursor, self._dropped = self._state[0:1], self._state[1:2]

  def rows_in_use(self):
    """Synchronises.  How many rows of the buffers hold a result."""
    return min(int(self._state[0]), self.capacity)

  def dropped(self):
    """Synchronises.  How many rows did not fit since the last reset()."""
    return int(self._state[1])

  def reset(self):
    self._state.zero_()


def stereo_forward(feature_net, stereo_net, left, right, output_cost_volume=False):
  """Reference train.py:19-22.  In eval mode the feature extractor is stateless and batch-independent (bit for bit), so
  both images pass it as one batch (half the launches); in train mode each image keeps its own BatchNorm statistics."""
  if not feature_net.training and left.shape == right.shape:
    both = feature_net(torch.cat([left, right]))
    left_feat, right_feat = both[:left.shape[0]], both[left.shape[0]:]
  else:
    left_feat, right_feat = feature_net(left), feature_net(right)
  return stereo_net(left, left_feat, right_feat, "l", output_cost_volume=output_cost_volume)


def eval_batches(feature_net, stereo_net, batches, num_images, input_scale):
  """Generator over (first_index, inputs, left, outputs): `batches` (any iterable of dicts with ``color_l/{s}`` and
  ``color_r/{s}``) through the networks in eval mode, each forward pass under no_grad and with output_cost_volume=True, until
  num_images images are in.  The grad mode is the consumer's own between the passes.  Each network's train/eval state is
  restored when the generator ends or is closed: a consumer that may leave early (an exception included) closes it, e.g. with
  contextlib.closing."""
  s = int(input_scale)
  f_training, s_training = feature_net.training, stereo_net.training
  feature_net.eval(); stereo_net.eval()
  seen = 0
  try:
    for inputs in batches:
      if seen >= num_images:
        break
      left = inputs["color_l/{}".format(s)].cuda()
      right = inputs["color_r/{}".format(s)].cuda()
      with torch.no_grad():
        outputs = stereo_forward(feature_net, stereo_net, left, right, output_cost_volume=True)
      yield seen, inputs, left, outputs
      seen += left.shape[0]
  finally:
    feature_net.train(f_training); stereo_net.train(s_training)
