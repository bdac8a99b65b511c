"""A plain float64 restatement of ONE launch each of the middle of the cost-aggregation chain, the four 3x3x3 32 -> 32 layers:
as_agg3d_fwd (csrc/agg3d.hip: training forward, eval forward and data gradient, three operand forms, three epilogues, the
contiguous and the column-strip form), as_conv32_fwd on the 3-D LDS route (conv3d_lds_kernel) and as_conv32_wgrad on the 3-D LDS
route (conv3d_wgrad_lds_kernel + the slab reduction); the bound of every output; the launch plans restated from the host code;
and the cases the GPU file (tests/test_gpu_agg3d_fp64.py) runs.  CPU only: nothing here imports the library.
tests/test_agg_ref_cpu.py holds the restatements to torch's float64 convolution, BatchNorm and autograd, brackets fp32
accumulations with the bounds, holds the restated plans to the library's host queries over a sweep, and shows that the cases tell
deliberately wrong restatements (MUTANTS) from the right one.

Tensors are channel-last: volumes are [B, D, H, W, 32] (a PCL interior); weights are torch's [co][ci][kd][kh][kw], tap
t = 9 kd + 3 kh + kw; the data gradient is the same sum over w.transpose(0, 1).flip(2, 3, 4) (as_conv32_pack_weights with
transpose_flip), without bias.

Bounds, derived and never fitted (U = 2^-24, gamma(n) = n U / (1 - n U)): a sum of n fp32 terms added in ANY order errs by at
most gamma(n) sum|terms|.
  z, g_x           gamma(865) (|bias| + sum |a| |w|): 864 products and the bias, whatever the order inside the matrix instruction.
  affine / partial operand forms: a = lrelu(fma(z_prev, scale, shift)) is tail_ref.operand's, with its per-voxel bound e_a
                   carried through conv(e_a, |w|).  The halo is zero, never lrelu(shift).
  a_out            its own roundings: the fused multiply-add, the product with the slope (the maximum of the two is exact) and
                   the slope's own fp32 value against 0.2: gamma(3) (|z_prev scale| + |shift|).  LeakyReLU is continuous: a sign
                   undecided at y ~ 0 moves a by no more than that.
  eval epilogue    y = lrelu(fma(acc, scale, shift)): LeakyReLU is 1-Lipschitz, so e_y = |scale| e_z + gamma(3) (|scale| (|z| + e_z) + |shift|).
  dW               gamma(B D H W (+ 1 with accumulate)) sum |x| |g| (+ |prior|);  db the same gamma with sum |g|.  The slab split,
                   the wave fold and the reduction's order do not enter.
  in-kernel merge  the state workgroup 0 publishes is judged with bn_ref.merge_bounds; a_out and z then from the PUBLISHED fp32
                   scale and shift, as the affine form."""
import numpy as np
import torch
import torch.nn.functional as F

import bn_ref as br
import tail_ref as tr
from tail_ref import U, gamma_n, SLOPE, TAPS, NAN, F64, ratio, geom_id, chan_scale    # noqa: F401

N_TERMS = 32 * 27 + 1
K_AOUT = 3                # the by-product's roundings: fma, slope product, the slope constant's fp32 value
K_EPI = 3                 # the eval epilogue's: the same three
CAP = 168                 # slabs of the 3-D LDS weight gradient at most
MAX_WS = 83               # widest (sub-)plane whose four runs fit in LDS


def _cdiv(a, b):
  return (a + b - 1) // b


# ----------------------------------------------------------------------------- as_agg3d_fwd: the plan (agg3d.hip, host part)
def agg_plan(geom):
  """None where as_agg3d_ok refuses; else dict(strips, Ws, tps (tiles per strip), tpp, npos, run, seg_len, nseg, units, per_xcd,
  grid).  Halo (1, 1, 1) assumed."""
  B, D, H, W = geom
  strips = 1 if W + 2 <= MAX_WS else _cdiv(W, 78)
  Ws = W + 2 if strips == 1 else (_cdiv(W, strips) + 2 + 7) // 8 * 8
  cw = W if strips == 1 else Ws - 2
  run = 130 + 2 * Ws + (7 if strips > 1 else 0)
  npos = (H - 1) * Ws + cw
  if min(B, D, H, W) < 1 or Ws < 34 or Ws > MAX_WS or Ws > W + 2 or npos < 128 or (H + 2) * Ws >= 65536 or run > 32 * 12:
    return None
  if _cdiv(run, 8) * 1024 * 4 + 4096 > 156 * 1024:
    return None
  tps = _cdiv(npos, 128)
  tpp = strips * tps
  cols = B * tpp
  best, best_cost = 1, 1e30
  for L in range(1, D + 1):
    cost = float(_cdiv(cols * _cdiv(D, L), 256)) * (L + 1.0)
    if cost < best_cost - 1e-9:
      best, best_cost = L, cost
  nseg = _cdiv(D, best)
  units = cols * nseg
  return dict(strips=strips, Ws=Ws, cw=cw, tps=tps, tpp=tpp, npos=npos, run=run, seg_len=best, nseg=nseg, units=units,
              per_xcd=_cdiv(units, 8), grid=8 * _cdiv(units, 8))


def plan_vector(p):
  """as_agg3d_plan's eight numbers"""
  return [p["strips"], p["Ws"], p["tps"], p["npos"], p["run"], p["seg_len"], p["nseg"], p["units"]]


def strip_origin(p, W, s):
  """(xs, dupc): the padded global column of strip column 0 — the last strip right-aligned — and the interior strip columns
  <= dupc that belong to the strip before"""
  Ws = p["Ws"]
  if p["strips"] == 1:
    return 0, 0
  xs = min(s * (Ws - 2), W + 2 - Ws)
  return xs, s * (Ws - 2) - xs


def plane_tiles(geom, mut=None):
  """owner [H, W] (int: the tile of the plane, strip-major, that counts the voxel in its moments: the first that writes it),
  writes [H, W] (how many tiles store it), halo_zero [H + 2, W + 2] (bool: halo voxels that a tile stores a zero to), last [H, W]
  (bool: written by a shifted-back last tile only).
  mut:  "overlap_late"  the overlap columns of a right-aligned strip are counted by that strip instead of the one before"""
  B, D, H, W = geom
  p = agg_plan(geom)
  Ws, first = p["Ws"], p["Ws"] + 1
  owner = np.full((H, W), -1, dtype=np.int64)
  writes = np.zeros((H, W), dtype=np.int64)
  last = np.zeros((H, W), dtype=bool)
  halo_zero = np.zeros((H + 2, W + 2), dtype=bool)
  for s in range(p["strips"]):
    xs, dupc = strip_origin(p, W, s)
    for t in range(p["tps"]):
      pos_new = first + 128 * t
      pos0 = min(pos_new, first + p["npos"] - 128)
      pos = pos0 + np.arange(128)
      yp, xp = pos // Ws, pos % Ws
      if p["strips"] == 1:
        inside = (xp >= 1) & (xp < 1 + W)
        fresh = inside & (pos >= pos_new)
        gx = xp
        halo_zero[yp[~inside], xp[~inside]] = True             # halo columns between rows are stored as zeros
      else:
        gx = xs + xp
        inside = (xp >= 1) & (xp <= Ws - 2) & (gx < 1 + W)
        fresh = inside & (pos >= pos_new) & (xp > dupc)
        if mut == "overlap_late":
          fresh = inside & (pos >= pos_new)
        if not bool(inside.all()):
          halo_zero[0, 0] = True                               # rows that are not kept go (as zeros) onto voxel 0 of the plane
      y, x = yp[inside] - 1, gx[inside] - 1
      np.add.at(writes, (y, x), 1)
      tile = s * p["tps"] + t
      fy, fx = yp[fresh] - 1, gx[fresh] - 1
      if mut == "overlap_late":
        owner[fy, fx] = tile
      else:
        assert bool((owner[fy, fx] == -1).all()), "a voxel counted twice"
        owner[fy, fx] = tile
      if pos0 < pos_new:
        last[fy, fx] = True
  return dict(owner=owner, writes=writes, halo_zero=halo_zero, last=last)


def unit_of(geom, tiles=None):
  """[B, D, H, W] (int64 tensor): the unit that owns each voxel, unit = ((b tpp + tile) nseg + d // seg_len)"""
  B, D, H, W = geom
  p = agg_plan(geom)
  tiles = tiles if tiles is not None else plane_tiles(geom)
  own = torch.from_numpy(tiles["owner"]).reshape(1, 1, H, W)
  b = torch.arange(B).reshape(B, 1, 1, 1)
  seg = (torch.arange(D) // p["seg_len"]).reshape(1, D, 1, 1)
  return (b * p["tpp"] + own) * p["nseg"] + seg


def partial_counts(geom, mut=None):
  """[grid]: the voxels each workgroup counts in its BatchNorm partial — workgroup blk runs unit (blk & 7) per_xcd + (blk >> 3);
  idle workgroups (unit >= units) write (0, 0, 0)"""
  p = agg_plan(geom)
  u = unit_of(geom, plane_tiles(geom, mut)).reshape(-1)
  per_unit = torch.bincount(u, minlength=p["units"])
  out = torch.zeros(p["grid"], dtype=torch.int64)
  for blk in range(p["grid"]):
    unit = (blk & 7) * p["per_xcd"] + (blk >> 3)
    if unit < p["units"]:
      out[blk] = per_unit[unit]
  return out


# ----------------------------------------------------------------------------- first generation and weight gradient: the plans
def lds3d_ok(geom):
  """conv3d_lds_applicable / conv3d_wgrad_lds_applicable for the 3x3x3 layer on halo (1, 1, 1): Wp >= 34, one full tile per
  plane, at most 64 DMA groups per run — Wp <= 191"""
  B, D, H, W = geom
  Wp = W + 2
  return Wp >= 34 and (H - 1) * Wp + W >= 128 and _cdiv(130 + 2 * Wp, 8) <= 64


def lds3d_tiles_per_plane(geom):
  B, D, H, W = geom
  return _cdiv((H - 1) * (W + 2) + W, 128)


def stat_parts(geom):
  """as_conv32_stat_parts: one partial per tile on the LDS route, else (27 taps: never split-K) per 128 voxels"""
  B, D, H, W = geom
  return B * D * lds3d_tiles_per_plane(geom) if lds3d_ok(geom) else _cdiv(B * D * H * W, 128)


def wgrad_generic_plan(geom):
  """conv32_wgrad_plan for 27 taps: (segments per row, chunks)"""
  B, D, H, W = geom
  groups, nsteps = 9, (W + 1) >> 1
  waves = B * D * H * groups
  nseg = 1
  if waves < 1024:
    nseg = max(min(_cdiv(2048, waves), _cdiv(nsteps, 32)), 1)
  seg_steps = _cdiv(_cdiv(nsteps, nseg), 8) * 8
  nseg = _cdiv(nsteps, seg_steps)
  rows = B * D * H * nseg
  want = min(_cdiv(4096, groups * 4), 512)
  rpc = max(_cdiv(rows, want), 4)
  return nseg, _cdiv(rows, rpc)


def wgrad_plan(geom):
  """dict(lds, tiles, slabs, segments (0 = an LDS kernel), workspace (floats))"""
  B, D, H, W = geom
  if lds3d_ok(geom):
    tiles = B * D * lds3d_tiles_per_plane(geom)
    slabs, seg = min(tiles, CAP), 0
  else:
    tiles = 0
    seg, slabs = wgrad_generic_plan(geom)
  return dict(lds=lds3d_ok(geom), tiles=tiles, slabs=slabs, segments=seg, workspace=slabs * 27 * 1024 + slabs * 32)


def wgrad_assign(block, ntiles, nchunks):
  """conv3d_wgrad_assign: (working, chunk, kd, extra tile or -1) of workgroup `block`"""
  xcd, q = block & 7, block >> 3
  i = q // 3
  per_xcd = (nchunks + 7) >> 3
  kd, chunk = q - 3 * i, xcd * per_xcd + i
  if chunk >= nchunks or i >= per_xcd:
    return False, chunk, kd, -1
  rank = xcd
  for r in range(i):
    rank += min((nchunks - r + per_xcd - 1) // per_xcd, 8)
  full = ntiles // nchunks
  extra = full * nchunks + rank if rank < ntiles - full * nchunks else -1
  return True, chunk, kd, extra


def wgrad_grid(nchunks):
  return 8 * _cdiv(nchunks, 8) * 3


def wgrad_coverage(ntiles, nchunks):
  """[ntiles, 3]: how often each (tile, kd) is walked by the launch's workgroups"""
  cov = np.zeros((ntiles, 3), dtype=np.int64)
  full = ntiles // nchunks
  for blk in range(wgrad_grid(nchunks)):
    ok, chunk, kd, extra = wgrad_assign(blk, ntiles, nchunks)
    if not ok:
      continue
    for k in range(full):
      cov[chunk + k * nchunks, kd] += 1
    if extra >= 0:
      cov[extra, kd] += 1
  return cov


def wgrad_tile_of(geom):
  """[B, D, H, W] (int64): the weight gradient's tile of each voxel — tiles of 128 positions from the first interior voxel, the
  last one ragged and NOT shifted back"""
  B, D, H, W = geom
  tpp = lds3d_tiles_per_plane(geom)
  pos = torch.arange(H).reshape(H, 1) * (W + 2) + torch.arange(W).reshape(1, W)
  plane = (torch.arange(B).reshape(B, 1) * D + torch.arange(D).reshape(1, D)).reshape(B, D, 1, 1)
  return plane * tpp + (pos // 128).reshape(1, 1, H, W)


# ----------------------------------------------------------------------------- the convolution
def pad_operand(a, fill=None, plane_fill=None):
  """[B, D + 2, H + 2, W + 2, 32]: a inside its zero halo.  fill / plane_fill ([32]): what a WRONG kernel would hold in the halo
  voxels of the interior planes / in the two halo planes"""
  ap = F.pad(a, (0, 0, 1, 1, 1, 1, 1, 1))
  if fill is not None:
    m = torch.ones(ap.shape[1:4], dtype=torch.bool)
    m[:, 1:-1, 1:-1] = False
    m[0], m[-1] = False, False
    ap[:, m] = fill.to(ap.dtype)
  if plane_fill is not None:
    ap[:, 0] = plane_fill.to(ap.dtype)
    ap[:, -1] = plane_fill.to(ap.dtype)
  return ap


def conv_sum(ap, w, bias=None, dtype=F64, mut=None):
  """z[b, d, y, x, co] = bias[co] + sum_{kd, kh, kw, ci} ap[b, d + kd, y + kh, x + kw, ci] w[co, ci, kd, kh, kw] over the PADDED
  operand ap, taps added in TAPS order (kd-major, the kernels' order).
  mut:  ("row_off", t) / ("plane_off", t)   tap t reads one row / one plane further down (zero beyond the padded volume)
        ("stale_fourth", seg_len)           an output plane other than the first of its segment reads, for kd = 2, the plane its
                                            ring slot was requested to replace three planes earlier (plane d in place of d + 3)"""
  B, Dp, Hp, Wp, _ = ap.shape
  D, H, W = Dp - 2, Hp - 2, Wp - 2
  kind, arg = mut if mut is not None else (None, None)
  x = F.pad(ap.to(dtype), (0, 0, 0, 0, 0, 1, 0, 1))
  wd = w.to(dtype)
  live = [t for t, (kd, kh, kw) in enumerate(TAPS) if bool(wd[:, :, kd, kh, kw].any())]     # (a single-tap case: the other taps add exact zeros)
  # "project, then shift": every voxel is projected once onto the live taps (32 products each), the taps are added in order
  wl = torch.stack([wd[:, :, TAPS[t][0], TAPS[t][1], TAPS[t][2]].t() for t in live], 1).reshape(32, 32 * len(live)) if live else None
  P = x @ wl if live else None
  out = torch.zeros(B, D, H, W, 32, dtype=dtype)
  if bias is not None:
    out = out + bias.to(dtype)
  for k, t in enumerate(live):
    kd, kh, kw = TAPS[t]
    dz = kd + (1 if kind == "plane_off" and arg == t else 0)
    dy = kh + (1 if kind == "row_off" and arg == t else 0)
    Pt = P[..., 32 * k:32 * k + 32]
    src = Pt[:, dz:dz + D, dy:dy + H, kw:kw + W]
    if kind == "stale_fourth" and kd == 2:
      src = src.clone()
      for d in range(D):
        if d % arg != 0:
          src[:, d] = Pt[:, d - 1, dy:dy + H, kw:kw + W]
    out = out + src
  return out


def transposed(w):
  """the data gradient's weights: g_x = conv(g, transposed(w))"""
  return w.transpose(0, 1).flip(2, 3, 4).contiguous()


def unwritten(z, geom, mut):
  """z with the voxels a wrong launch would never store set to NaN.
  mut:  ("no_shift_back", 1)   the last tile of a (sub-)plane is not shifted back to end at npos: what it alone writes is missing
        ("skip_round", n)      units from n on (the second round of 256 workgroups) never run"""
  kind, arg = mut
  B, D, H, W = geom
  z = z.clone()
  if kind == "no_shift_back":
    z[:, :, torch.from_numpy(plane_tiles(geom)["last"])] = NAN
  if kind == "skip_round":
    z[unit_of(geom) >= arg] = NAN
  return z


def strip_conv(a, w, bias, geom, mut=None):
  """The strip form restated strip by strip: every strip convolves its own window of Ws padded columns (its two outer columns
  are its halo: real voxels of the neighbour, or the plane's halo) and stores its interior columns at xs + x'; an overlap column
  is stored by both strips with the same value.
  mut:  "left_aligned"   the last strip's window is taken left-aligned (columns from strip (Ws - 2), zero beyond the plane)
                         while its outputs are stored right-aligned"""
  B, D, H, W = geom
  p = agg_plan(geom)
  Ws = p["Ws"]
  ap = F.pad(pad_operand(a.double()), (0, 0, 0, Ws))
  out = torch.full((B, D, H, W, 32), NAN, dtype=F64)
  for s in range(p["strips"]):
    xs, dupc = strip_origin(p, W, s)
    src = s * (Ws - 2) if mut == "left_aligned" else xs
    win = ap[:, :, :, src:src + Ws]
    zs = conv_sum(win, w, bias)                                # [B, D, H, Ws - 2, 32]: strip columns 1 .. Ws - 2
    n = min(Ws - 2, W - xs)
    out[:, :, :, xs:xs + n] = zs[:, :, :, :n]
  return out


# ----------------------------------------------------------------------------- restatement + bound
def forward(x, w, bias=None, scale=None, shift=None, ep_scale=None, ep_shift=None):
  """One launch on the fp32 values it read.  a (the operand: x, or lrelu(fma(x, scale, shift)) inside a zero halo), z = bias +
  conv(a, w) and e_z; with scale: e_a (carried into e_z) and e_a_out, the by-product's own bound; with ep_scale: y =
  lrelu(z ep_scale + ep_shift) and e_y"""
  a, e_a = tr.operand(x, scale, shift)
  aw = w.double().abs()
  z = conv_sum(pad_operand(a), w, bias)
  e_z = gamma_n(N_TERMS) * conv_sum(pad_operand(a.abs()), aw, bias.abs() if bias is not None else None)
  out = dict(a=a, e_a=e_a)
  if scale is not None:
    e_z = e_z + conv_sum(pad_operand(e_a), aw)
    out["e_a_out"] = gamma_n(K_AOUT) * ((x.double() * scale.double()).abs() + shift.double().abs())
  out.update(z=z, e_z=e_z)
  if ep_scale is not None:
    sc, sh = ep_scale.double(), ep_shift.double()
    y = z * sc + sh
    out["y"] = torch.where(y > 0, y, y * SLOPE)
    out["e_y"] = sc.abs() * e_z + gamma_n(K_EPI) * (sc.abs() * (z.abs() + e_z) + sh.abs())
  return out


def data_gradient(g, w):
  """g_x = conv(g, transposed(w)) and its bound gamma(864) ... the bias-free sum: gamma(865) keeps the rule uniform (and is larger)"""
  wt = transposed(w)
  return dict(g_x=conv_sum(pad_operand(g.double()), wt), e_g_x=gamma_n(N_TERMS) * conv_sum(pad_operand(g.double().abs()), wt.abs()))


def wgrad_sum(x, g, dtype=F64, mut=None):
  """dW[co, ci, kd, kh, kw] = sum_p x[p + tap, ci] g[p, co] (x zero outside the volume), db[co] = sum_p g[p, co].
  mut:  ("skip_extra", 1)     the tiles beyond the full rounds (tile >= (tiles // slabs) slabs) are never walked
        ("drop_chunks", CAP)  one chunk per tile, but only the first CAP slabs are reduced: tiles from CAP on are lost
        ("swap_kd", 1)        the slabs of kd = 0 and kd = 2 change places
        ("db_per_kd", 1)      every kd's workgroup adds its bias sum: db three times over"""
  B, D, H, W, _ = x.shape
  geom = (B, D, H, W)
  kind, arg = mut if mut is not None else (None, None)
  gd = g.to(dtype)
  if kind in ("skip_extra", "drop_chunks"):
    p = wgrad_plan(geom)
    lim = (p["tiles"] // p["slabs"]) * p["slabs"] if kind == "skip_extra" else arg
    gd = gd * (wgrad_tile_of(geom) < lim).to(dtype)[..., None]
  xp = F.pad(x.to(dtype), (0, 0, 1, 1, 1, 1, 1, 1))
  g2 = gd.reshape(-1, 32)
  dW = torch.zeros(32, 32, 3, 3, 3, dtype=dtype)
  for (kd, kh, kw) in TAPS:
    dW[:, :, kd, kh, kw] = g2.t() @ xp[:, kd:kd + D, kh:kh + H, kw:kw + W].reshape(-1, 32)
  db = g2.sum(0)
  if kind == "swap_kd":
    dW = dW.flip(2)
  if kind == "db_per_kd":
    db = 3.0 * db
  return dW, db


def weight_gradient(x, g, dW0=None, db0=None):
  """dW, db and their bounds  gamma(N) wgrad(|x|, |g|),  gamma(N) sum|g|,  N = B D H W; with dW0 / db0 (accumulate = 1) the value
  already there is one more term"""
  N = x.shape[0] * x.shape[1] * x.shape[2] * x.shape[3]
  dW, db = wgrad_sum(x, g)
  aW, ab = wgrad_sum(x.abs(), g.abs())
  if dW0 is not None:
    N += 1
    dW, db = dW + dW0.double(), db + db0.double()
    aW, ab = aW + dW0.double().abs(), ab + db0.double().abs()
  return dict(dW=dW, db=db, e_dW=gamma_n(N) * aW, e_db=gamma_n(N) * ab)


def merged_state(cnt, mean, m2, gamma, beta, rm, rv):
  """the BatchNorm state from fp32 partials (cnt [P], mean / m2 [P, 32]) in float64, and bn_ref.merge_bounds for the consumer merge"""
  n, mu, q = br.chan_merge64(cnt, mean, m2)
  ref = br.bn_state64(n, mu, q, gamma, beta, rm, rv)
  return ref, br.merge_bounds(cnt, mean, m2, gamma, ref, c=int(cnt.numel()) + 32)


# ----------------------------------------------------------------------------- the geometries the GPU file runs
# as_agg3d_fwd, contiguous form: (B, D, H, W) -> what as_agg3d_plan must answer for (seg_len, nseg, units, grid)
AGG_GEOMS = [
  ((1, 1, 2, 63), dict(seg_len=1, nseg=1, units=1, grid=8)),        # one tile of exactly 128 positions; 7 idle workgroups; D = 1
  ((1, 1, 4, 32), dict(seg_len=1, nseg=1, units=2, grid=8)),        # Wp = 34, the minimum; npos 134: the last tile shifted back by 122
  ((1, 2, 4, 33), dict(seg_len=1, nseg=2, units=4, grid=8)),        # D = 2: the fourth-plane request is skipped
  ((1, 3, 4, 33), dict(seg_len=1, nseg=3, units=6, grid=8)),        # D = 3
  ((2, 3, 5, 32), dict(seg_len=1, nseg=3, units=12, grid=16)),
  ((3, 5, 9, 40), dict(seg_len=1, nseg=5, units=45, grid=48)),
  ((2, 7, 6, 81), dict(seg_len=1, nseg=7, units=56, grid=56)),      # Wp = 83, the maximum; the grid an exact multiple of 8
  ((40, 7, 2, 63), dict(seg_len=2, nseg=4, units=160, grid=160)),   # segments of two planes, the last one ragged (one plane)
  ((90, 7, 2, 63), dict(seg_len=4, nseg=2, units=180, grid=184)),   # segments of four planes, the last of three
  ((257, 1, 2, 63), dict(seg_len=1, nseg=1, units=257, grid=264)),  # a second round of 256
]
# strip form: -> (strips, Ws, overlap columns of the last strip)
STRIP_GEOMS = [
  ((1, 2, 3, 82), dict(strips=2, Ws=48, dupc=10)),
  ((1, 2, 3, 120), dict(strips=2, Ws=64, dupc=4)),                  # the second strip right-aligned with 4 overlap columns
  ((1, 2, 2, 156), dict(strips=2, Ws=80, dupc=0)),
  ((1, 2, 2, 200), dict(strips=3, Ws=72, dupc=10)),                 # three strips, 12 units on a grid of 16
  ((1, 1, 2, 189), dict(strips=3, Ws=72, dupc=21)),
]
EXACT_GEOMS = [(1, 1, 4, 32), (1, 3, 4, 33), (1, 2, 3, 120), (40, 7, 2, 63)]
# as_conv32_fwd on the 3-D LDS route: -> whether conv3d_lds_kernel takes it
FIRST_GEN_GEOMS = [((1, 1, 2, 63), True), ((1, 1, 4, 32), True), ((3, 5, 9, 40), True), ((1, 1, 2, 189), True), ((1, 1, 2, 190), False)]
# as_conv32_wgrad: -> (tiles, slabs); tiles 0: the generic kernel
WGRAD_GEOMS = [
  ((1, 1, 2, 63), (1, 1)),          # one tile, one chunk, seven padding chunks
  ((1, 9, 2, 63), (9, 9)),          # per_xcd 2: chunks 9 .. 15 are padding
  ((1, 3, 4, 33), (6, 6)),          # two tiles per plane, the last unshifted and ragged; clamped DMA groups
  ((1, 167, 2, 63), (167, 167)),
  ((1, 168, 2, 63), (168, 168)),    # the cap exactly
  ((1, 169, 2, 63), (169, 168)),    # one extra tile
  ((3, 113, 2, 63), (339, 168)),    # two full rounds and three extra tiles
  ((33, 8, 2, 63), (264, 168)),
  ((1, 2, 3, 120), (6, 6)),
  ((1, 1, 2, 189), (3, 3)),         # Wp = 191, the last width the LDS kernels take
  ((1, 1, 2, 190), (0, 0)),         # the generic kernel
]
WGRAD_EXACT_GEOMS = [(1, 1, 2, 63), (1, 3, 4, 33), (1, 169, 2, 63)]


# ----------------------------------------------------------------------------- the cases
def _gen(seed):
  return torch.Generator().manual_seed(seed)


def _seed(geom, k):
  B, D, H, W = geom
  return 100003 * k + 7 * B + 1009 * D + 131 * H + W


def seam_voxels(geom):
  """(y, x) on either side of the first tile seam of a contiguous plane — positions 127 and 128 counted from the first interior
  voxel, each moved off a halo column away from the seam; the last two voxels where the plane has one tile"""
  B, D, H, W = geom
  if (H - 1) * (W + 2) + W <= 128:
    return [(H - 1, W - 2), (H - 1, W - 1)]
  out = []
  for pos, step in ((127, -1), (128, 1)):
    while pos % (W + 2) >= W:
      pos += step
    out.append(divmod(pos, W + 2))
  return out


def add_sentinels(t):
  """tail_ref's +-1e4 on the first and last plane, row and column, and one more on either side of the first tile seam"""
  B, D, H, W, C = t.shape
  tr.add_sentinels(t)
  for k, (y, x) in enumerate(seam_voxels((B, D, H, W))):
    t[B - 1, D // 2, y, x, (7 * k + 1) % C] = 1e4 * (-1.0) ** k
  return t


def random_weights(seed):
  w = torch.randn(32, 32, 3, 3, 3, generator=_gen(seed)) / 864 ** 0.5
  return w, torch.randn(32, generator=_gen(seed + 1)) * 0.1


def bn_affine(seed):
  """gamma in 0.5 .. 1.5 and |beta| in 0.2 .. 0.5: lrelu(shift) in a halo voxel would be seen"""
  g = _gen(seed)
  gamma = 0.5 + torch.rand(32, generator=g)
  beta = (0.2 + 0.3 * torch.rand(32, generator=g)) * (1.0 - 2.0 * (torch.arange(32) % 2))
  return gamma, beta


def random_case(geom):
  """x and g (a gradient) with sentinels, dense weights and bias, an affine (scale, shift) for the operand and the eval epilogue,
  gamma / beta / running statistics for the BatchNorm that is still in partials"""
  B, D, H, W = geom
  x = add_sentinels(torch.randn(B, D, H, W, 32, generator=_gen(_seed(geom, 1))) * chan_scale())
  g = add_sentinels(torch.randn(B, D, H, W, 32, generator=_gen(_seed(geom, 2))) * chan_scale())
  w, b = random_weights(_seed(geom, 3))
  scale, shift = bn_affine(_seed(geom, 4))
  gamma, beta = bn_affine(_seed(geom, 5))
  gen = _gen(_seed(geom, 6))
  return dict(x=x, g=g, w=w, b=b, scale=scale, shift=shift, gamma=gamma, beta=beta, rm=torch.randn(32, generator=gen) * 0.1,
              rv=torch.rand(32, generator=gen) + 0.5)


def tap_weights(t):
  """One tap times a channel permutation: w[co, perm[co], tap] = +-2^k.  The forward, and the data gradient over the transposed
  packing, are then copies scaled by a power of two: exact for any x"""
  kd, kh, kw = TAPS[t]
  w = torch.zeros(32, 32, 3, 3, 3)
  co = torch.arange(32)
  perm = torch.randperm(32, generator=_gen(50 + t))
  w[co, perm, kd, kh, kw] = torch.pow(2.0, (co % 7 - 3).float()) * (1.0 - 2.0 * (co % 2))
  return w


def integer_case(geom):
  """x, w, g in {-2 .. 2}, a whole-number bias: every partial sum is an integer below 2^24, exact in fp32 in any order"""
  B, D, H, W = geom
  gen = _gen(_seed(geom, 7))
  x = torch.randint(-2, 3, (B, D, H, W, 32), generator=gen).float()
  g = torch.randint(-2, 3, (B, D, H, W, 32), generator=gen).float()
  w = torch.randint(-2, 3, (32, 32, 3, 3, 3), generator=gen).float()
  return dict(x=x, g=g, w=w, b=torch.randint(-5, 6, (32,), generator=gen).float())


IMPULSE_SPOTS = ["seam", "last_col", "rows", "planes", "extra"]


def _tile_voxel(geom, tile):
  """the first interior voxel (b, d, y, x) of the weight gradient's tile"""
  B, D, H, W = geom
  tpp = lds3d_tiles_per_plane(geom)
  plane, tt = divmod(tile, tpp)
  pos = 128 * tt
  while pos % (W + 2) >= W:
    pos += 1
  return (plane // D, plane % D, pos // (W + 2), pos % (W + 2))


def impulse_case(geom, spot):
  """g is +-2^k per channel at TWO voxels and x holds multiples of 2^-8 below 16: every dW entry is a sum of at most two products
  that fp32 holds exactly in any order, db of two powers of two.  Spots: "seam" positions 127 and 128 of a plane (seam_voxels);
  "last_col" the last column of the first and the last row; "rows" the first row and the last; "planes" plane 0 and plane D - 1
  (kd reaches a halo plane); "extra" the first extra tile (the last tile where there is none) and the last chunk's first tile"""
  B, D, H, W = geom
  gen = _gen(_seed(geom, 8))
  x = (torch.randn(B, D, H, W, 32, generator=gen) * 256.0).round().clamp(-4095, 4095) / 256.0
  p = wgrad_plan(geom)
  if spot == "extra":
    full = p["tiles"] // p["slabs"]
    t_extra = full * p["slabs"] if p["tiles"] > full * p["slabs"] else p["tiles"] - 1
    spots = [_tile_voxel(geom, t_extra), _tile_voxel(geom, p["slabs"] - 1)]
    if spots[0] == spots[1]:                                   # (no extra tile: the last tile is the last chunk's; its last voxel)
      spots[1] = (B - 1, D - 1, H - 1, W - 1)
  else:
    (ys, xs_), (ye, xe) = seam_voxels(geom)
    spots = {"seam": [(0, D // 2, ys, xs_), (0, D // 2, ye, xe)],
             "last_col": [(0, 0, 0, W - 1), (B - 1, D - 1, H - 1, W - 1)],
             "rows": [(0, D // 2, 0, W // 3), (B - 1, D // 2, H - 1, (2 * W) // 3)],
             "planes": [(0, 0, H // 2, W // 2), (B - 1, D - 1, H // 2, W // 3)]}[spot]
  co = torch.arange(32)
  g = torch.zeros(B, D, H, W, 32)
  g[spots[0]] = torch.pow(2.0, (co % 5 - 2).float()) * (1.0 - 2.0 * (co % 2))
  g[spots[1]] = g[spots[1]] + torch.pow(2.0, (co % 3 - 1).float()) * (1.0 - 2.0 * ((co // 2) % 2))
  return dict(x=x, g=g, spots=spots)


def prior(exact, seed=77):
  """what an accumulating launch finds in dW and db (multiples of 2^-8 for the exact families)"""
  gen = _gen(seed)
  d0, b0 = torch.randn(32, 32, 3, 3, 3, generator=gen), torch.randn(32, generator=gen)
  if exact:
    d0, b0 = (d0 * 256).round() / 256, (b0 * 256).round() / 256
  return d0, b0


# ----------------------------------------------------------------------------- deliberately wrong restatements
# name -> (kind, mut); tests/test_agg_ref_cpu.py shows that a named case catches each of them
MUTANTS = {
  "a tap one row off (tap 5)": ("conv", ("row_off", 5)),
  "a tap one row off (tap 24)": ("conv", ("row_off", 24)),
  "a tap one plane off (tap 13)": ("conv", ("plane_off", 13)),
  "the last tile not shifted back": ("unwritten", ("no_shift_back", 1)),
  "a unit beyond 256 skipped": ("unwritten", ("skip_round", 256)),
  "the second strip left-aligned instead of right-aligned": ("strip", "left_aligned"),
  "the overlap columns taken from the wrong strip": ("owner", "overlap_late"),
  "a halo voxel activated as lrelu(shift)": ("halo", "voxel"),
  "a halo plane activated": ("halo", "plane"),
  "a segment's fourth plane served stale": ("conv", ("stale_fourth", None)),
  "the weight gradient's extra tile skipped": ("wgrad", ("skip_extra", 1)),
  "kd planes 0 and 2 swapped": ("wgrad", ("swap_kd", 1)),
  "a chunk from 168 on dropped": ("wgrad", ("drop_chunks", CAP)),
  "the bias gradient counted once per kd": ("wgrad", ("db_per_kd", 1)),
}
