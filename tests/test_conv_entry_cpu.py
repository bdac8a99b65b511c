"""The host side of the generic and thin-input convolution entry points (csrc/conv_entry.hip): what each one refuses.

As tests/test_layer_entry_cpu.py: every case carries ONE defect and is refused on the host before any HIP call, so no
GPU is needed and none of the fabricated addresses is ever dereferenced.  The geometry of every other argument is one
the route under test accepts (its query is asked first), so a case that was NOT refused would be a launch: each case
asserts status -1, that the message begins with the name of the entry point that was called, and that it carries the
phrase of that refusal.  (as_conv32_dgrad_s2_packed reports as "as_conv32_dgrad_s2", the name of the pair of entry
points it belongs to; the phrases are those every form of a refusal carries.)
"""
import ctypes

import pytest

from adaptive_stereo import _native as nat

B = 2


def pcl(H, W, ph, pw, D=1, pd=0, b=B):
  return nat.Pcl(b, D, H, W, pd, ph, pw)


S33 = dict(kd=1, kh=3, kw=3, pad_d=0, pad_h=1, pad_w=1, dil=1, stride=1)
S55 = dict(kd=1, kh=5, kw=5, pad_d=0, pad_h=2, pad_w=2, dil=1, stride=2)


def shape(d):
  return nat.ConvShape(d["kd"], d["kh"], d["kw"], d["pad_d"], d["pad_h"], d["pad_w"], d["dil"], d["stride"])


_FWD32 = "x gin w bias z gout s epilogue ep_scale ep_shift slope residual stat_mean stat_m2 stat_cnt stream".split()
_FWD4 = "x gin w bias z gout s epilogue ep_scale ep_shift slope stat_mean stat_m2 stat_cnt stream".split()
_BNAPPLY32 = "x gin g_a z gout s scale shift mean coef slope g_z dW db accumulate workspace stream".split()
_BNAPPLY4 = "x gin g_a z gout s Cin scale shift mean coef slope g_z dW db accumulate workspace stream".split()
_PROJ4 = "x gin g_a z gout s Cin scale shift mean coef slope w_proj h dW db accumulate workspace stream".split()
_BN_PTRS = ["x", "g_a", "z", "scale", "shift", "mean", "coef", "dW", "workspace"]

# entry point -> argument list in C order, the geometry its route accepts (input extent and halo, output halo, shape), the
# query that says so (None: the generic route takes every legal geometry) and the answer expected, the required pointers, the
# phrase of a null pointer, the prefix of its messages where that is not its own name
ENTRIES = {
  # the LDS-staged 3x3 route (full-resolution layers) ...
  "as_conv32_fwd": dict(args=_FWD32, geo=(40, 256, 8, 8, 8, 8, S33), ok="as_conv32_bnbwd_parts", required=["x", "w", "z"],
                        epilogue=True),
  # ... and the generic kernels (the strided head)
  "as_conv32_fwd/generic": dict(args=_FWD32, geo=(48, 156, 2, 2, 1, 1, S55), ok=None, required=["x", "w", "z"], epilogue=True),
  "as_conv32_fwd_bnbwd": dict(args="x gin w z gout s residual bn_z bn_scale bn_shift bn_mean slope bn_workspace stream".split(),
                              geo=(40, 256, 8, 8, 8, 8, S33), ok="as_conv32_bnbwd_parts", unsupported_ok="as_conv32_bnbwd_parts",
                              required=["x", "w", "z", "bn_z", "bn_scale", "bn_shift", "bn_mean", "bn_workspace"],
                              aligned="bn_workspace"),
  "as_conv32_wgrad": dict(args="x gin gz gout s dW db accumulate workspace stream".split(), geo=(40, 256, 8, 8, 8, 8, S33),
                          ok=None, required=["x", "gz", "dW", "workspace"]),
  "as_conv32_wgrad/generic": dict(args="x gin gz gout s dW db accumulate workspace stream".split(),
                                  geo=(48, 156, 2, 2, 1, 1, S55), ok=None, required=["x", "gz", "dW", "workspace"]),
  "as_conv32_wgrad_bnapply": dict(args=_BNAPPLY32, geo=(1536, 256, 8, 8, 8, 8, S33), ok="as_conv32_wgrad_bnapply_ok",
                                  unsupported_ok="as_conv32_wgrad_bnapply_ok", required=_BN_PTRS + ["g_z"]),
  "as_conv4_fwd": dict(args=_FWD4, geo=(40, 256, 1, 1, 8, 8, S33), ok="as_conv4_wgrad_bnapply_ok", required=["x", "w", "z"],
                       epilogue=True, thin=True),
  "as_conv4_fwd/generic": dict(args=_FWD4, geo=(48, 156, 2, 2, 1, 1, S55), ok=None, required=["x", "w", "z"], epilogue=True,
                               thin=True),
  "as_conv4_wgrad": dict(args="x gin gz gout s Cin dW db accumulate workspace stream".split(), geo=(40, 256, 1, 1, 8, 8, S33),
                         ok="as_conv4_wgrad_bnapply_ok", required=["x", "gz", "dW", "workspace"], thin=True, null="bad argument"),
  "as_conv4_wgrad/generic": dict(args="x gin gz gout s Cin dW db accumulate workspace stream".split(),
                                 geo=(48, 156, 2, 2, 1, 1, S55), ok=None, required=["x", "gz", "dW", "workspace"], thin=True,
                                 null="bad argument"),
  "as_conv4_wgrad_bnapply": dict(args=_BNAPPLY4, geo=(40, 256, 1, 1, 8, 8, S33), ok="as_conv4_wgrad_bnapply_ok",
                                 unsupported_ok="as_conv4_wgrad_bnapply_ok", required=_BN_PTRS + ["g_z"], thin=True,
                                 null="bad argument"),
  "as_conv4_wgrad_bnapply_proj": dict(args=_PROJ4, geo=(40, 256, 1, 1, 8, 8, S33), ok="as_conv4_wgrad_bnapply_ok",
                                      unsupported_ok="as_conv4_wgrad_bnapply_ok", required=_BN_PTRS + ["w_proj", "h"], thin=True,
                                      null="bad argument"),
}
_NOT_POINTERS = ("gin", "gout", "s", "slope", "accumulate", "epilogue", "Cin", "stream")


def _geometry(geo, **over):
  H, W, ph, pw, oph, opw, sd = geo
  sd = dict(sd, **over.pop("shape", {}))
  Ho = (H + 2 * sd["pad_h"] - sd["dil"] * (sd["kh"] - 1) - 1) // sd["stride"] + 1
  Wo = (W + 2 * sd["pad_w"] - sd["dil"] * (sd["kw"] - 1) - 1) // sd["stride"] + 1
  return pcl(H, W, ph, pw), pcl(Ho, Wo, oph, opw), shape(sd)


def _refused(key, phrase, gin=None, gout=None, s=None, check_ok=True, **changes):
  """Calls the entry point with fabricated distinct non-null addresses, `changes` applied, and checks the refusal."""
  lib = nat.load()
  e = ENTRIES[key]
  name = key.split("/")[0]
  g0 = _geometry(e["geo"])
  if e["ok"] and check_ok:                       # the defect under test is the only one: the route takes this geometry
    assert getattr(lib, e["ok"])(*[ctypes.byref(v) for v in g0]) >= 1
  gin, gout, s = gin or g0[0], gout or g0[1], s or g0[2]
  vals = {}
  for i, a in enumerate(e["args"]):
    vals[a] = {"gin": gin, "gout": gout, "s": s, "slope": 0.2, "accumulate": 0, "epilogue": 0, "Cin": 4, "stream": None,
               "ep_scale": None, "ep_shift": None, "residual": None, "bias": None, "db": None}.get(a, 0x100000 * (i + 1))
  for a, v in changes.items():
    assert a in vals, a
    vals[a] = v
  argv = [ctypes.byref(vals[a]) if isinstance(vals[a], ctypes.Structure) else vals[a] for a in e["args"]]
  assert getattr(lib, name)(*argv) == -1, "%s was not refused: %s" % (name, changes)
  msg = lib.as_last_error().decode()
  assert msg.startswith(name) and phrase in msg, msg


def _keys(pred):
  return [k for k, e in sorted(ENTRIES.items()) if pred(e)]


@pytest.mark.parametrize("key,arg", [(k, a) for k, e in sorted(ENTRIES.items()) for a in e["required"]])
def test_null_pointer_is_refused(key, arg):
  _refused(key, ENTRIES[key].get("null", "null pointer"), **{arg: None})


@pytest.mark.parametrize("key,arg", [(k, a) for k in sorted(ENTRIES) for a in ("gin", "gout", "s")])
def test_null_geometry_is_refused(key, arg):
  lib = nat.load()
  e = ENTRIES[key]
  name = key.split("/")[0]
  gin, gout, s = _geometry(e["geo"])
  vals = {a: {"gin": gin, "gout": gout, "s": s, "slope": 0.2, "accumulate": 0, "epilogue": 0, "Cin": 4,
              "stream": None}.get(a, 0x100000 * (i + 1)) for i, a in enumerate(e["args"])}
  vals[arg] = None
  argv = [ctypes.byref(vals[a]) if isinstance(vals[a], ctypes.Structure) else vals[a] for a in e["args"]]
  assert getattr(lib, name)(*argv) == -1
  msg = lib.as_last_error().decode()
  assert msg.startswith(name) and "bad geometry" in msg, msg


@pytest.mark.parametrize("missing", ["ep_scale", "ep_shift"])
@pytest.mark.parametrize("key", _keys(lambda e: e.get("epilogue")))
def test_epilogue_1_without_scale_or_shift_is_refused(key, missing):
  both = {"ep_scale": 0x7000000, "ep_shift": 0x7100000, "stat_mean": None, "stat_m2": None, "stat_cnt": None}
  both[missing] = None
  _refused(key, "bad epilogue arguments", epilogue=1, **both)


@pytest.mark.parametrize("key", _keys(lambda e: e.get("epilogue")))
def test_unknown_epilogue_is_refused(key):
  _refused(key, "bad epilogue arguments", epilogue=2, ep_scale=0x7000000, ep_shift=0x7100000)


@pytest.mark.parametrize("given", [(0,), (1,), (2,), (0, 1), (0, 2), (1, 2)])
@pytest.mark.parametrize("key", _keys(lambda e: e.get("epilogue")))
def test_one_or_two_moment_arrays_are_refused(key, given):
  stats = ("stat_mean", "stat_m2", "stat_cnt")
  _refused(key, "bad epilogue arguments", **{a: None for i, a in enumerate(stats) if i not in given})


@pytest.mark.parametrize("key", sorted(ENTRIES))
def test_batch_mismatch_is_refused(key):
  # (the thin-input family names the check of its 4-float input, which holds the batch rule, the 32-channel family the rule)
  phrase = "bad input extent" if ENTRIES[key].get("thin") else "batch"
  gin, gout, _ = _geometry(ENTRIES[key]["geo"])
  gin.B, gout.B = B + 1, B + 1
  _refused(key, phrase, gout=gout)
  _refused(key, phrase, gin=gin)


@pytest.mark.parametrize("axis,delta", [("H", 1), ("H", -1), ("W", 1), ("W", -1)])
@pytest.mark.parametrize("key", sorted(ENTRIES))
def test_output_extent_off_by_one_is_refused(key, axis, delta):
  _, gout, _ = _geometry(ENTRIES[key]["geo"])
  setattr(gout, axis, getattr(gout, axis) + delta)
  _refused(key, "output extent", gout=gout)


@pytest.mark.parametrize("odd", [False, True])
@pytest.mark.parametrize("axis", ["ph", "pw"])
@pytest.mark.parametrize("key", sorted(ENTRIES))
def test_input_halo_one_too_small_is_refused(key, axis, odd):
  """The halo is the same on both sides of an axis, and the taps reach `padding` voxels beyond the top / left edge.  Beyond
  the bottom / right edge a stride-1 layer reaches as far; a 5x5 stride-2 layer reaches 1 over an even extent and 2 over an
  odd one, so both parities are asked: a halo of padding - 1 is refused in each."""
  H, W, ph, pw, oph, opw, sd = ENTRIES[key]["geo"]
  gin, gout, s = _geometry((H + odd, W + odd, sd["pad_h"], sd["pad_w"], oph, opw, sd))
  setattr(gin, axis, getattr(gin, axis) - 1)
  _refused(key, "input halo", gin=gin, gout=gout, s=s, check_ok=False)


@pytest.mark.parametrize("key", _keys(lambda e: e.get("thin")))
def test_3d_geometry_for_a_thin_input_is_refused(key):
  H, W, ph, pw, oph, opw, sd = ENTRIES[key]["geo"]
  gin, gout, s = _geometry(ENTRIES[key]["geo"])
  _refused(key, "2-D only", gin=pcl(H, W, ph, pw, D=2), gout=pcl(gout.H, gout.W, oph, opw, D=2))
  _refused(key, "2-D only", gin=pcl(H, W, ph, pw, pd=1))
  _refused(key, "2-D only", gout=pcl(gout.H, gout.W, oph, opw, pd=1))
  s3 = shape(dict(sd, kd=3, pad_d=1))
  _refused(key, "2-D only", s=s3)


@pytest.mark.parametrize("cin", [0, 5, -1])
@pytest.mark.parametrize("key", _keys(lambda e: "Cin" in e["args"]))
def test_cin_outside_1_4_is_refused(key, cin):
  _refused(key, "bad argument", Cin=cin)


@pytest.mark.parametrize("key", _keys(lambda e: e.get("unsupported_ok")))
def test_unsupported_configuration_is_refused(key):
  """A legal convolution the fused form does not exist for: its query answers 0 and the entry point refuses."""
  lib = nat.load()
  e = ENTRIES[key]
  H, W, ph, pw, oph, opw, sd = e["geo"]
  geo = (24, 100, 2, 2, 2, 2, dict(S33, dil=2, pad_h=2, pad_w=2))       # dilation 2 (thin input), W < 128 (32 channels)
  gin, gout, s = _geometry(geo)
  assert getattr(lib, e["unsupported_ok"])(ctypes.byref(gin), ctypes.byref(gout), ctypes.byref(s)) == 0
  _refused(key, "not supported", gin=gin, gout=gout, s=s, check_ok=False)


def test_small_launch_has_no_fused_bnapply():
  # the LDS weight gradient takes the layer, but its form with stage 3 of the BatchNorm backward needs a chip-filling launch
  lib = nat.load()
  gin, gout, s = _geometry((40, 256, 8, 8, 8, 8, S33))
  assert lib.as_conv32_wgrad_bnapply_ok(ctypes.byref(gin), ctypes.byref(gout), ctypes.byref(s)) == 0
  _refused("as_conv32_wgrad_bnapply", "not supported", gin=gin, gout=gout, s=s, check_ok=False)


def test_unaligned_batchnorm_workspace_is_refused():
  _refused("as_conv32_fwd_bnbwd", "8-byte aligned", bn_workspace=0x7000004)


# ---- the entry points without a convolution shape -----------------------------------------------------------------------
def _call(name, *argv):
  lib = nat.load()
  assert getattr(lib, name)(*[ctypes.byref(a) if isinstance(a, ctypes.Structure) else a for a in argv]) == -1, name
  return lib.as_last_error().decode()


_GZ, _GX = (94, 311, 1, 1), (188, 621, 2, 2)        # the head's first stride-2 32->32 layer at four pairs


def _dgrad(gz=0x100000, ggz=None, packed=0x200000, gx=0x300000, ggx=None):
  ggz = ggz or pcl(*_GZ, b=4)
  ggx = ggx or pcl(*_GX, b=4)
  msg = _call("as_conv32_dgrad_s2_packed", gz, ggz, packed, gx, ggx, None)
  assert msg.startswith("as_conv32_dgrad_s2"), msg
  return msg


def test_dgrad_s2_packed_refusals():
  lib = nat.load()
  assert lib.as_conv32_s2_dgrad_ok(ctypes.byref(pcl(*_GZ, b=4)), ctypes.byref(pcl(*_GX, b=4))) == 1
  for arg in ("gz", "packed", "gx"):
    assert "bad argument" in _dgrad(**{arg: None})
  assert "bad argument" in _call("as_conv32_dgrad_s2_packed", 0x100000, None, 0x200000, 0x300000, pcl(*_GX, b=4), None)
  assert "bad argument" in _call("as_conv32_dgrad_s2_packed", 0x100000, pcl(*_GZ, b=4), 0x200000, 0x300000, None, None)
  assert "equal batch" in _dgrad(ggz=pcl(*_GZ, b=3))
  assert "2-D" in _dgrad(ggz=pcl(*_GZ, b=4, D=2), ggx=pcl(*_GX, b=4, D=2))
  for dh, dw in ((1, 0), (-1, 0), (0, 1), (0, -1)):
    assert "extent" in _dgrad(ggz=pcl(_GZ[0] + dh, _GZ[1] + dw, 1, 1, b=4))
  assert "halo" in _dgrad(ggz=pcl(_GZ[0], _GZ[1], 0, 1, b=4))
  assert "halo" in _dgrad(ggz=pcl(_GZ[0], _GZ[1], 1, 0, b=4))


def test_conv4_pack_weights_refusals():
  s = shape(S33)
  for argv in ((None, 4, 0x200000, s, None), (0x100000, 4, None, s, None), (0x100000, 4, 0x200000, None, None),
               (0x100000, 0, 0x200000, s, None), (0x100000, 5, 0x200000, s, None)):
    msg = _call("as_conv4_pack_weights", *argv)
    assert msg.startswith("as_conv4_pack_weights") and "bad argument" in msg, msg
  for taps in (shape(dict(S33, kh=7, kw=7)), shape(dict(S33, kh=0))):
    msg = _call("as_conv4_pack_weights", 0x100000, 4, 0x200000, taps, None)
    assert msg.startswith("as_conv4_pack_weights") and "taps unsupported" in msg, msg


def test_pack_in4_refusals():
  g = pcl(40, 256, 1, 1)
  for bad in (None, pcl(40, 256, 1, 1, D=2), pcl(40, 256, 1, 1, pd=1), pcl(40, 256, 1, 1, b=0), pcl(0, 256, 1, 1),
              pcl(40, 0, 1, 1)):
    msg = _call("as_pack_in4", 0x100000, 0x200000, 3, 0x300000, bad, None)
    assert msg.startswith("as_pack_in4") and "bad geometry" in msg, msg
  for argv in ((0x100000, None, 3, 0x300000, g, None), (0x100000, 0x200000, 3, None, g, None),
               (0x100000, 0x200000, 0, 0x300000, g, None), (0x100000, 0x200000, 4, 0x300000, g, None),
               (None, 0x200000, 5, 0x300000, g, None)):
    msg = _call("as_pack_in4", *argv)
    assert msg.startswith("as_pack_in4") and "bad argument" in msg, msg


def test_a_thin_input_too_large_for_32_channels_is_not_refused_for_its_size():
  """A PCL4 input holds 4 floats per pixel: one that would pass 2^31 elements at 32 floats per voxel is legal, and the
  geometry checks let it through (the call is refused for its null operand, which is tested after them)."""
  gin, gout = pcl(8000, 8380, 8, 8, b=1), pcl(8000, 8380, 0, 0, b=1)
  assert gin.numel() >= 2 ** 31 > gout.numel()
  msg = _call("as_conv4_fwd", None, gin, 0x200000, None, 0x300000, gout, shape(S33), 0, None, None, 0.2, None, None, None,
              None)
  assert msg.startswith("as_conv4_fwd") and "null pointer" in msg, msg
