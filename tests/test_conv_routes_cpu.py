"""The host queries of the generic and thin-input convolution entry points, held to a recorded table.

Every query below answers from the same route decision its entry point launches by (csrc/conv_entry.hip), so a table of
their answers over both sides of every predicate pins the decisions: which kernel takes a layer, how many BatchNorm
partials it writes, how large a weight-gradient workspace is.  The table (tests/conv_routes_parent.json) is this
library's own output, recorded by `python tests/test_conv_routes_cpu.py --record` before the decisions were gathered in
one place; a route change re-records it on purpose.  None of the queries makes a HIP call: no GPU is needed.
"""
import ctypes
import json
import os
import sys

if __name__ == "__main__":
  sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "adaptive-stereo-icra-2021_amd"))

from adaptive_stereo import _native as nat

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "conv_routes_parent.json")

S33 = (1, 3, 3, 0, 1, 1, 1, 1)            # (kd, kh, kw, pad_d, pad_h, pad_w, dil, stride)
S55_S2 = (1, 5, 5, 0, 2, 2, 1, 2)
S333 = (3, 3, 3, 1, 1, 1, 1, 1)


def s33(dil=1, pad=None, stride=1):
  pad = dil if pad is None else pad
  return (1, 3, 3, 0, pad, pad, dil, stride)


def _cases():
  """(name, B, D, H, W, input halo (pd, ph, pw), output halo, shape).  H, W are the INPUT extent; the output extent is
  the convolution's."""
  c = []

  def add(name, B, D, H, W, hin, hout, s):
    c.append((name, B, D, H, W, tuple(hin), tuple(hout), tuple(s)))

  # conv32_lds_applicable: W 127 / 128, input pw 7 / 8, ph = dil - 1 / dil, dil 8 / 9, pad != dil, stride 2; output pw 7 / 8
  for W in (127, 128, 129, 256):
    add("lds2d_W%d" % W, 2, 1, 40, W, (0, 8, 8), (0, 8, 8), s33())
  for pw in (7, 8):
    add("lds2d_in_pw%d" % pw, 2, 1, 40, 256, (0, 8, pw), (0, 8, 8), s33())
    add("lds2d_out_pw%d" % pw, 2, 1, 40, 256, (0, 8, 8), (0, 8, pw), s33())
  for dil in (1, 2, 4, 8):
    add("lds2d_dil%d_ph_short" % dil, 2, 1, 40, 256, (0, dil - 1, 8), (0, 8, 8), s33(dil)) if dil > 1 else None
    add("lds2d_dil%d_ph_exact" % dil, 2, 1, 40, 256, (0, dil, 8), (0, 8, 8), s33(dil))
  add("lds2d_dil9", 2, 1, 40, 256, (0, 9, 9), (0, 9, 9), s33(9))
  add("lds2d_pad_ne_dil", 2, 1, 40, 256, (0, 8, 8), (0, 8, 8), s33(2, pad=1))
  add("lds2d_stride2", 2, 1, 40, 256, (0, 8, 8), (0, 8, 8), s33(1, stride=2))
  # ... its weight gradient: both sides of the launch that fills the chip (3072 tiles), the full-resolution layer
  for H in (1535, 1536):
    add("wgrad_lds_tiles_H%d" % H, 1, 1, H, 256, (0, 8, 8), (0, 8, 8), s33(2))
  add("wgrad_lds_full_res", 4, 1, 375, 1242, (0, 8, 8), (0, 8, 8), s33(2))
  add("wgrad_lds_one_pair", 1, 1, 96, 256, (0, 8, 8), (0, 8, 8), s33())

  # conv3d_lds_applicable / conv3d_wgrad_lds_applicable: pad 0 on one axis, differing halos, the LDS bound on the padded row
  add("lds3d_base", 1, 12, 24, 78, (1, 1, 1), (1, 1, 1), S333)
  add("lds3d_four_pairs", 4, 12, 24, 78, (1, 1, 1), (1, 1, 1), S333)
  for i, h in enumerate(((0, 1, 1), (1, 0, 1), (1, 1, 0))):
    add("lds3d_pad0_axis%d" % i, 1, 12, 24, 78, h, h, S333)
  add("lds3d_halos_differ", 1, 12, 24, 78, (1, 1, 2), (1, 1, 1), S333)
  add("lds3d_halos_differ_out", 1, 12, 24, 78, (1, 1, 1), (1, 2, 1), S333)
  for W in (189, 190):                      # padded row 191 / 192: the staged run of 130 + 2 Wp voxels in 64 KB of LDS
    add("lds3d_lds_bound_W%d" % W, 1, 6, 24, W, (1, 1, 1), (1, 1, 1), S333)
  for W in (31, 32):                        # padded row 33 / 34
    add("lds3d_Wp_W%d" % W, 1, 6, 24, W, (1, 1, 1), (1, 1, 1), S333)
  for H in (2, 3):                          # less / more than one full 128-position tile per plane at W = 62
    add("lds3d_one_tile_H%d" % H, 1, 6, H, 62, (1, 1, 1), (1, 1, 1), S333)
  add("lds3d_dil2", 1, 12, 24, 78, (2, 2, 2), (2, 2, 2), (3, 3, 3, 2, 2, 2, 2, 1))
  add("lds3d_many_tiles", 2, 48, 47, 156, (1, 1, 1), (1, 1, 1), S333)

  # split-K: M = 32768 / 32769 and 16384 / 16385 at 9 taps, 16384 / 16385 and 8192 / 8193 at 25 taps
  for M in (16384, 16385, 32768, 32769):
    add("splitk_9taps_M%d" % M, 1, 1, 1, M, (0, 1, 1), (0, 1, 1), s33())
  for M in (8192, 8193, 16384, 16385):
    add("splitk_25taps_M%d" % M, 1, 1, 1, 2 * M, (0, 2, 2), (0, 1, 1), S55_S2)
  add("splitk_9taps_small_map", 4, 1, 24, 78, (0, 1, 1), (0, 1, 1), s33())
  add("splitk_27taps", 1, 4, 6, 20, (1, 1, 1), (1, 1, 1), S333)

  # staged 32->32 stride-2 forward / data gradient: 1023 / 1024 tiles, halo 1 / 2 (forward) and 0 / 1 (gradient)
  add("s2_tiles_1023", 1, 1, 186, 704, (0, 2, 2), (0, 1, 1), S55_S2)        # 93 rows x 11 segments
  add("s2_tiles_1024", 1, 1, 128, 1024, (0, 2, 2), (0, 1, 1), S55_S2)       # 64 rows x 16 segments
  add("s2_odd_extent", 4, 1, 187, 621, (0, 2, 2), (0, 1, 1), S55_S2)
  for h in (1, 2, 3):
    add("s2_in_halo%d" % h, 1, 1, 128, 1024, (0, max(h, 2), h), (0, 1, 1), S55_S2)
    add("s2_in_halo_rows%d" % h, 1, 1, 128, 1024, (0, h, max(h, 2)), (0, 1, 1), S55_S2) if h < 2 else None
  for h in (0, 1, 2):
    add("s2_out_halo%d" % h, 1, 1, 128, 1024, (0, 2, 2), (0, h, h), S55_S2)
  add("s2_out_halo_ph0_pw1", 1, 1, 128, 1024, (0, 2, 2), (0, 0, 1), S55_S2)
  # 1024 tiles of 8 voxels: split-K (M = 8192 <= 16384) and the staged rows both apply: split-K has precedence
  add("s2_and_splitk", 4, 1, 512, 16, (0, 2, 2), (0, 1, 1), S55_S2)
  add("s2_head_level1", 4, 1, 188, 621, (0, 2, 2), (0, 2, 2), S55_S2)
  add("s2_head_level2", 4, 1, 94, 311, (0, 2, 2), (0, 2, 2), S55_S2)
  add("s2_head_level3", 4, 1, 47, 156, (0, 2, 2), (0, 2, 2), S55_S2)

  # generic weight gradient: both sides of the 1024-wave rule at T = 9, 25, 27, a width capped by the shortest segment
  for H in (341, 342):
    add("wgrad_9taps_H%d" % H, 1, 1, H, 100, (0, 1, 1), (0, 1, 1), s33())                # 3 tap groups per row
  for H in (408, 410):
    add("wgrad_25taps_H%d" % H, 1, 1, H, 200, (0, 2, 2), (0, 1, 1), S55_S2)              # 5 tap groups, 204 / 205 rows
  for D in (113, 114):
    add("wgrad_27taps_D%d" % D, 1, D, 1, 20, (1, 1, 1), (1, 1, 1), S333)                 # 9 tap groups per row
  for W in (20, 64, 65, 100, 127, 640):
    add("wgrad_seg_cap_W%d" % W, 1, 1, 4, W, (0, 9, 9), (0, 9, 9), s33(9))               # 12 waves: segments capped by W
  add("wgrad_small_map", 4, 1, 24, 78, (0, 1, 1), (0, 1, 1), s33())
  add("wgrad_3d_generic", 1, 12, 24, 30, (1, 1, 1), (1, 1, 1), S333)
  add("wgrad_1x1", 2, 1, 24, 78, (0, 0, 0), (0, 1, 1), (1, 1, 1, 0, 0, 0, 1, 1))

  # 4-channel rows: W 31 / 32, padded width 63 / 64, halo 0 / 1
  for W in (31, 32, 33):
    add("c4_rows_W%d" % W, 2, 1, 20, W, (0, 16, 16), (0, 1, 1), S33)
  for W, pw in ((61, 1), (62, 1), (33, 15), (32, 16)):
    add("c4_rows_padded_W%d_pw%d" % (W, pw), 2, 1, 20, W, (0, 1, pw), (0, 1, 1), S33)
  for h in ((0, 0, 1), (0, 1, 0), (0, 0, 0), (0, 1, 1)):
    add("c4_rows_halo_%d%d" % (h[1], h[2]), 2, 1, 20, 200, h, (0, 1, 1), S33)
  add("c4_rows_full_res", 4, 1, 375, 1242, (0, 1, 1), (0, 8, 8), S33)
  add("c4_rows_dil2", 2, 1, 20, 200, (0, 2, 2), (0, 1, 1), s33(2))
  # 4-channel staged 5x5 stride 2: 4095 / 4096 tiles, halo 1 / 2
  add("c4_s2_tiles_4095", 1, 1, 130, 4032, (0, 2, 2), (0, 2, 2), S55_S2)     # 65 rows x 63 segments
  add("c4_s2_tiles_4096", 1, 1, 128, 4096, (0, 2, 2), (0, 2, 2), S55_S2)     # 64 rows x 64 segments
  for h in ((0, 1, 2), (0, 2, 1), (0, 2, 2), (0, 3, 3)):
    add("c4_s2_halo_%d%d" % (h[1], h[2]), 1, 1, 128, 4096, h, (0, 2, 2), S55_S2)
  add("c4_s2_full_res", 4, 1, 375, 1242, (0, 2, 2), (0, 2, 2), S55_S2)
  # 4-channel generic weight gradient: NB 2 (9 taps), NB 4 (25 taps); 5x5 stride 2 with the staged plan the larger
  # workspace (few units: 512 slots make more chunks than 768) and with the generic plan the larger (many units)
  add("c4_wgrad_nb2", 2, 1, 20, 200, (0, 2, 2), (0, 1, 1), s33(2))
  add("c4_wgrad_nb2_stride2", 2, 1, 40, 200, (0, 1, 1), (0, 1, 1), s33(1, stride=2))
  add("c4_wgrad_nb4_stride1", 2, 1, 20, 200, (0, 2, 2), (0, 1, 1), (1, 5, 5, 0, 2, 2, 1, 1))
  for H in (8, 64, 256, 375, 750, 1500, 3000):
    add("c4_wgrad_s2_plans_H%d" % H, 4, 1, H, 1242, (0, 2, 2), (0, 2, 2), S55_S2)
  add("c4_wgrad_1x1", 2, 1, 20, 200, (0, 0, 0), (0, 1, 1), (1, 1, 1, 0, 0, 0, 1, 1))
  add("c4_wgrad_7x7", 2, 1, 20, 200, (0, 3, 3), (0, 1, 1), (1, 7, 7, 0, 3, 3, 1, 1))     # 49 taps: beyond AS_MAX_TAPS
  return [x for x in c if x is not None]


CASES = _cases()
QUERIES = ("as_conv32_stat_parts", "as_conv32_s2_fwd_ok", "as_conv32_bnbwd_parts", "as_conv32_num_blocks",
           "as_conv32_wgrad_segments", "as_conv32_wgrad_workspace", "as_conv32_wgrad_bnapply_ok", "as_conv32_s2_dgrad_ok",
           "as_conv4_stat_parts", "as_conv4_s2_ok", "as_conv4_wgrad_workspace", "as_conv4_wgrad_bnapply_ok")


def _geometry(case):
  _, B, D, H, W, hin, hout, s = case
  kd, kh, kw, pad_d, pad_h, pad_w, dil, stride = s
  Ho = (H + 2 * pad_h - dil * (kh - 1) - 1) // stride + 1
  Wo = (W + 2 * pad_w - dil * (kw - 1) - 1) // stride + 1
  Do = D + 2 * pad_d - dil * (kd - 1) if kd > 1 else D
  return nat.Pcl(B, D, H, W, *hin), nat.Pcl(B, Do, Ho, Wo, *hout), nat.ConvShape(*s)


def answers(case):
  """Every query's answer for one case, with both library switches at 0 and then at 1 (restored afterwards)."""
  lib = nat.load()
  gin, gout, s = _geometry(case)
  i, o, sp = ctypes.byref(gin), ctypes.byref(gout), ctypes.byref(s)
  argv = {"as_conv32_num_blocks": (o,), "as_conv32_s2_dgrad_ok": (o, i), "as_conv4_wgrad_workspace": (o, sp)}
  rows = []
  prev = lib.as_conv32_s2_enable(-1), lib.as_conv4_s2_enable(-1)
  try:
    for on in (0, 1):
      lib.as_conv32_s2_enable(on)
      lib.as_conv4_s2_enable(on)
      rows.append([int(getattr(lib, q)(*argv.get(q, (i, o, sp)))) for q in QUERIES])
  finally:
    lib.as_conv32_s2_enable(prev[0])
    lib.as_conv4_s2_enable(prev[1])
  return rows


def test_case_names_are_unique_and_the_table_covers_them():
  names = [c[0] for c in CASES]
  assert len(set(names)) == len(names)
  with open(TABLE) as f:
    table = json.load(f)
  assert table["queries"] == list(QUERIES)
  assert sorted(table["rows"]) == sorted(names)


def test_queries_answer_as_recorded():
  with open(TABLE) as f:
    table = json.load(f)
  wrong = []
  for case in CASES:
    got, want = answers(case), table["rows"][case[0]]
    for on in (0, 1):
      for q, g, w in zip(QUERIES, got[on], want[on]):
        if g != w:
          wrong.append("%s, switches %d: %s answers %d, recorded %d" % (case[0], on, q, g, w))
  assert not wrong, "\n".join(wrong)


def test_the_table_holds_both_sides_of_every_route():
  """The recorded answers themselves show each route taken and refused (a list that lost a side would pin nothing)."""
  with open(TABLE) as f:
    rows = json.load(f)["rows"]
  col = {q: i for i, q in enumerate(QUERIES)}

  def seen(q, on):
    return {r[on][col[q]] for r in rows.values()}

  for q in ("as_conv32_s2_fwd_ok", "as_conv32_s2_dgrad_ok", "as_conv4_s2_ok"):
    assert {0, 1} <= seen(q, 1) and 1 not in seen(q, 0), q        # the switch turns the staged routes off
  for q in ("as_conv32_wgrad_bnapply_ok", "as_conv4_wgrad_bnapply_ok"):
    assert {0, 1} <= seen(q, 1), q
  assert 0 in seen("as_conv32_bnbwd_parts", 1) and max(seen("as_conv32_bnbwd_parts", 1)) > 0
  assert 0 in seen("as_conv32_wgrad_segments", 1) and max(seen("as_conv32_wgrad_segments", 1)) > 1
  # split-K's precedence over the staged rows: one partial per 32 voxels although the staged shape test holds
  r = rows["s2_and_splitk"][1]
  assert r[col["as_conv32_s2_fwd_ok"]] == 0 and r[col["as_conv32_stat_parts"]] == 4 * 256 * 8 // 32
  # the 4-channel workspace is the larger plan's whatever the switch says
  for r in rows.values():
    assert r[0][col["as_conv4_wgrad_workspace"]] == r[1][col["as_conv4_wgrad_workspace"]]


if __name__ == "__main__":
  if sys.argv[1:] != ["--record"]:
    sys.exit("usage: python tests/test_conv_routes_cpu.py --record")
  with open(TABLE, "w") as f:
    f.write('{"queries": %s,\n "rows": {\n' % json.dumps(list(QUERIES)))
    f.write(",\n".join('  %s: %s' % (json.dumps(c[0]), json.dumps(answers(c))) for c in CASES))
    f.write("\n }}\n")
  print("recorded %d cases" % len(CASES))
