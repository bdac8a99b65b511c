"""The host side of the full-resolution 3x3 32->32 layer entry points (csrc/conv32_layer.hip): what each one refuses.

Every case carries ONE defect and is refused on the host before any HIP call, so no GPU is needed and none of the
fabricated addresses is ever dereferenced.  The geometry is one each route's own _ok query accepts (asked below; no
memory of that size exists), so a case that was NOT refused would be a launch: each case therefore asserts status -1,
that the message names the entry point that was called, and that it carries the phrase of that refusal.
"""
import ctypes
import math

import pytest

from adaptive_stereo import _native as nat

B, H, W, DIL, HALO = 4, 375, 1242, 2, 8


def _pcl(w=W, ph=HALO, pw=HALO):
  return nat.Pcl(B, 1, H, w, 0, ph, pw)


def _shape(dil=DIL):
  return nat.ConvShape(1, 3, 3, 0, dil, dil, dil, 1)


# Argument lists in C order.  Plain names are pointers; "gin" / "gout" / "g" geometries, "s" the shape, "slope" a float,
# "accumulate" / "residual" ints, "stream" the (null) stream.
_FWD = ("z_prev a_prevprev in_scale in_shift a_out gin w bias slope z gout s stat_mean stat_m2 stat_cnt stream").split()
_BWD = ("x gin g_a z gout s wt scale shift mean coef slope next_z next_scale next_shift next_mean g_x dW db accumulate "
        "next_bn_workspace workspace stream").split()
_BWD_GZ = _BWD[:16] + ["g_z"] + _BWD[16:]
_DATA = ("g_a z g s wt scale shift mean coef slope next_z next_scale next_shift next_mean g_z g_x next_bn_workspace "
         "stream").split()
_DATA_PTRS = [a for a in _DATA if a not in ("g", "s", "slope", "stream")]
_DATA_ALIAS = [("g_x", "g_a"), ("g_x", "z"), ("g_z", "g_a"), ("g_z", "z"), ("g_z", "g_x"), ("g_z", "next_z"), ("g_x", "next_z")]
_BWD_PTRS = [a for a in _BWD if a not in ("gin", "gout", "s", "slope", "db", "accumulate", "stream")]
_FWD_PTRS = ["z_prev", "in_scale", "in_shift", "a_out", "w", "z"]
_FWD_ALIAS = [("a_out", "z_prev"), ("a_out", "a_prevprev"), ("z", "z_prev"), ("z", "a_out"), ("z", "a_prevprev")]

# entry point -> its _ok query, argument list, what the parent refuses: required pointers, slope checked, moments,
# the aliasing pairs it names (first := second), the 8-byte aligned BatchNorm workspace
ENTRIES = {
  "as_conv32_act_fwd": dict(ok="as_conv32_act_ok", args=_FWD, required=_FWD_PTRS, slope=True, moments=True, alias=_FWD_ALIAS),
  "as_conv32_wino_fwd": dict(ok="as_conv32_wino_ok", args=_FWD, required=_FWD_PTRS, slope=True, moments=True, alias=_FWD_ALIAS),
  "as_conv32_wino_eval": dict(ok="as_conv32_wino_ok", args="x g s w bias scale shift slope residual out stream".split(),
                              required=["x", "w", "scale", "shift", "out"], slope=True, alias=[("out", "x")]),
  "as_conv32_wino_bwd_data": dict(ok="as_conv32_wino_ok", args=_DATA, required=_DATA_PTRS, slope=True, alias=_DATA_ALIAS,
                                  aligned=True),
  "as_conv32_wino_bwd_filter": dict(ok="as_conv32_wino_ok", args="x g_z g s dW db accumulate workspace stream".split(),
                                    required=["x", "g_z", "dW", "workspace"]),
  "as_conv32_wino_bwd": dict(ok="as_conv32_wino_ok", args=_BWD_GZ, required=["x", "dW", "workspace"] + _DATA_PTRS, slope=True,
                             alias=[("g_x", "x"), ("g_z", "x")] + _DATA_ALIAS, aligned=True),
  "as_conv32_wino_bwd_fused": dict(ok="as_conv32_wino_ok", args=_BWD, required=_BWD_PTRS, slope=True,
                                   alias=[("g_x", "g_a"), ("g_x", "z"), ("g_x", "x"), ("g_x", "next_z")], aligned=True),
  "as_conv32_bwd_fused": dict(ok="as_conv32_bwd_fused_ok", args=_BWD, required=_BWD_PTRS, slope=False,
                              alias=[("g_x", "g_a"), ("g_x", "x"), ("g_x", "z")], aligned=True),
}
_NOT_POINTERS = ("gin", "gout", "g", "s", "slope", "accumulate", "residual", "stream")


def _refused(name, phrase, **changes):
  """Calls `name` with fabricated distinct non-null addresses, `changes` applied, and checks the refusal."""
  lib = nat.load()
  e = ENTRIES[name]
  gin, gout, s = changes.pop("gin", _pcl()), changes.pop("gout", _pcl()), changes.pop("s", _shape())
  if not changes.pop("unsupported", False):      # the defect under test is the only one: the route takes this geometry
    assert getattr(lib, e["ok"])(ctypes.byref(_pcl()), ctypes.byref(_pcl()), ctypes.byref(_shape())) == 1
  vals = {}
  for i, a in enumerate(e["args"]):
    vals[a] = {"gin": gin, "gout": gout, "g": gout, "s": s, "slope": 0.2, "accumulate": 0, "residual": 0,
               "stream": None}.get(a, 0x100000 * (i + 1))
  for a, v in changes.items():
    assert a in vals and a not in _NOT_POINTERS or a == "slope", a
    vals[a] = vals[v] if isinstance(v, str) else v
  argv = [ctypes.byref(vals[a]) if isinstance(vals[a], ctypes.Structure) else vals[a] for a in e["args"]]
  assert getattr(lib, name)(*argv) == -1, "%s was not refused: %s" % (name, changes)
  msg = lib.as_last_error().decode()
  assert msg.startswith(name) and phrase in msg, msg


def _cases(key):
  return [(n, x) for n, e in sorted(ENTRIES.items()) for x in (e.get(key) or [])]


@pytest.mark.parametrize("name,arg", _cases("required"))
def test_null_pointer_is_refused(name, arg):
  _refused(name, "null pointer", **{arg: None})


@pytest.mark.parametrize("given", [(0,), (1,), (2,), (0, 1), (0, 2), (1, 2)])
@pytest.mark.parametrize("name", [n for n, e in sorted(ENTRIES.items()) if e.get("moments")])
def test_one_or_two_moment_arrays_are_refused(name, given):
  stats = ("stat_mean", "stat_m2", "stat_cnt")
  _refused(name, "all three", **{a: None for i, a in enumerate(stats) if i not in given})


@pytest.mark.parametrize("slope", [0.0, 1.0, -0.5, math.nan])
@pytest.mark.parametrize("name", [n for n, e in sorted(ENTRIES.items()) if e.get("slope")])
def test_slope_outside_0_1_is_refused(name, slope):
  _refused(name, "slope", slope=slope)


@pytest.mark.parametrize("name,pair", _cases("alias"))
def test_aliasing_is_refused(name, pair):
  _refused(name, "alias", **{pair[0]: pair[1]})


@pytest.mark.parametrize("name", [n for n, e in sorted(ENTRIES.items()) if e.get("aligned")])
def test_batchnorm_workspace_with_bit_2_set_is_refused(name):
  _refused(name, "8-byte aligned", next_bn_workspace=0x7000004)


@pytest.mark.parametrize("name", [n for n, e in sorted(ENTRIES.items()) if "gin" in e["args"]])
def test_input_in_another_padded_geometry_is_refused(name):
  # (the halo is still large enough for the taps: only the route's own test objects)
  _refused(name, "not supported", gin=_pcl(pw=2 * HALO), unsupported=True)
  _refused(name, "not supported", gin=_pcl(ph=2 * HALO), unsupported=True)


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_unsupported_configuration_is_refused(name):
  lib = nat.load()
  g, s = _pcl(w=63), _shape(dil=3)
  assert getattr(lib, ENTRIES[name]["ok"])(ctypes.byref(g), ctypes.byref(g), ctypes.byref(s)) == 0
  _refused(name, "not supported", gin=g, gout=_pcl(w=63), s=s, unsupported=True)


def test_queries():
  lib = nat.load()
  g, s = _pcl(), _shape()
  for ok in ("as_conv32_act_ok", "as_conv32_wino_ok", "as_conv32_bwd_fused_ok"):
    assert getattr(lib, ok)(ctypes.byref(g), ctypes.byref(g), ctypes.byref(s)) == 1
    assert getattr(lib, ok)(None, ctypes.byref(g), ctypes.byref(s)) == -1
    assert getattr(lib, ok)(ctypes.byref(g), ctypes.byref(g), None) == -1
  for parts in ("as_conv32_act_parts", "as_conv32_wino_parts", "as_conv32_wino_bwd_parts", "as_conv32_wino_bwd_fused_parts",
                "as_conv32_bwd_fused_parts"):
    assert getattr(lib, parts)() >= 1
  # a workspace holds one [9][32][32] weight slab and one [32] bias slab per workgroup of the weight-gradient launch
  assert lib.as_conv32_wino_bwd_fused_workspace() == lib.as_conv32_wino_bwd_fused_parts() * (9 * 1024 + 32)
  assert lib.as_conv32_bwd_fused_workspace() == lib.as_conv32_bwd_fused_parts() * (9 * 1024 + 32)
  assert lib.as_conv32_wino_bwd_workspace() > 0 and lib.as_conv32_wino_bwd_workspace() % (9 * 1024 + 32) == 0
  prev = lib.as_conv32_wino_bwd_generation(0)              # out of range: a query
  try:
    assert prev in (1, 2, 3)
    assert lib.as_conv32_wino_bwd_generation(1) == prev and lib.as_conv32_wino_bwd_generation(7) == 1
  finally:
    lib.as_conv32_wino_bwd_generation(prev)
  assert lib.as_conv32_wino_bwd_generation(0) == prev
