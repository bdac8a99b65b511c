"""What is particular to ONE launch each of the 2-D row-segment 32 -> 32 kernels (csrc/conv32_lds.hip: the nine forward flavours of
conv32_lds_body<MODE, RES>, conv32_wgrad_lds_kernel, conv32_wgrad_lds2_kernel<APPLY>) behind as_conv32_fwd, as_conv32_fwd_bnbwd,
as_conv32_wgrad and as_conv32_wgrad_bnapply: the tiling restated as plain functions of (B, H, W, grid), the owner map the moments
and the next BatchNorm's sums follow, the route decisions of csrc/conv_entry.hip for these shapes, the bound of every output and
the cases tests/test_gpu_lds2d_fp64.py runs.  The layer arithmetic and the bound forms are tests/wino_ref.py's (conv_direct,
wgrad_direct, act_chain, gz_chain, judge_gz, gamma, ratio, the scatter sums; the K * U * S forms of the moments and sums) — not
copied.  CPU only as far as the library goes: nothing here imports it; every function works on the device of its operands.
tests/test_lds2d_ref_cpu.py holds the restatements to torch, to the library's read-only queries and to their MUTANTS.

Tensors are channel-last interiors [B, H, W, 32], weights torch's [co][ci][3][3].

TILING (tile_coords, conv32_lds_body's loop head; the weight-gradient kernels share the banding)
  a tile is (image, row, 128-column segment): tiles_per_row = ceil(W / 128), tile t -> row t / tiles_per_row (image row / H, row
  row % H), x_new = 128 (t % tiles_per_row), x0 = min(x_new, W - 128): the last segment of a ragged row is shifted LEFT to end at
  W; it computes and stores its first dup = x_new - x0 columns a second time (equal values) and the moments (MODE 0) and the next
  BatchNorm's sums (MODE 3) skip them — a tile OWNS the columns [x_new, min(x_new + 128, W)).  The weight-gradient kernels do NOT
  shift: x0 = x_new, and the gradient operand beyond W reads as zero (the row's right halo: needs output pw >= 8 and ZERO halos).
  Banding: tiles_per_band = ceil(nt / 8), wg_per_xcd = grid / 8, workgroup b takes tiles (b & 7) band + (b >> 3) + k wg_per_xcd
  below min(((b & 7) + 1) band, nt).  grid: conv32_lds_grid = min(8 ceil(nt / 8), 512) forward; the weight gradient's slabs
  min(8 ceil(ceil(nt / 16) / 8), 512), or 256 from 3072 tiles on (conv32_wgrad_lds2_kernel).

BOUNDS, counted from the code, never fitted (u = 2^-24, gamma(n) = n u / (1 - n u), the form of wino_ref):
  z, g_x          gamma(288 + r) S, S = sum |x| |w| over the 288 products + |bias| (+ |residual|): the accumulator starts as the
                  bias (exact) and takes 144 two-term matrix steps, one rounding per term; r = 1 with a residual.  Split-K and the
                  direct kernel (W < 128) add the same 288 terms in another order: the same bound.
  eval            + 3: scale and shift (2, or 1 fused), the slope (1); on |scale| S + |shift| (+ |residual|).  max(y, slope y)
                  is continuous in y: no element is undecided here.
  moments k       wino_ref's lane model with n_l = 16 * the most tiles of a workgroup, over the pixels the owner map gives k;
                  count exact.  Flat partials of split-K (32 voxels) and the direct kernel (128): two passes —
                  e_mean = gamma(21) sum|z| / n (16 per lane, the half merge, 3 wave adds, the division),
                  e_M2 = gamma(26) (M2 + n e_mean^2) + n e_mean^2 (z - mean rounded, squared, summed the same way).
  next sums k     wino_ref's: per lane fp32 sums of n_l terms, an exact double sum of 8; + (1 - slope) |g_x| (|z - mean|) of every
                  element undecided on y_next.
  dW, db          gamma(n1 + n_w + n_r + a) S_w: n1 = 32 * the most tiles of a workgroup (16 steps of 2 terms per tile; 16 *
                  for the 8-wave kernel), n_w = 3 (7) wave sums, n_r = ceil(slabs / 16) + 16 (wgrad_reduce_kernel: 16 slices, then
                  their sum), a = 1 when accumulating; S_w = sum |x| |g_z|.  db: 16 (8) adds per tile and lane, the half
                  merge, 3 (7) wave adds, n_r.  The generic kernel (output pw < 8, W < 128): gamma(B H W + 1): n terms in any order.
  g_z (APPLY)     wino_ref.gz_chain / judge_gz.

EXACT CASES.  Every launch only multiplies and adds: with wino_ref.exact_case's small integers every sum stays far below 2^24
quanta (exact_headroom) and the launch must equal float64 bit for bit."""
import torch
import torch.nn.functional as F

import wino_ref as wr
from wino_ref import U, F64, gamma, ratio, conv_direct, wgrad_direct, act_chain, gz_chain, judge_gz, f32, case, exact_case, \
    EXACT_WEIGHTS, geom_id  # noqa: F401  (the GPU file takes them from here)

SEG = 128
MAX_WG = 512
LDS2_TILES = 256 * 12
N_K = 288
SPLITK_MAX_M = 32768

MUTANTS = ("drop_tap", "tap_dm1", "dup_twice", "dup_off_1", "band_off_1", "res_before_act", "skip_row", "g_wrapped")


# ----------------------------------------------------------------------------- tiling
def tiles_per_row(W):
  return -(-W // SEG)


def ntiles(B, H, W):
  return B * H * tiles_per_row(W)


def tile_coords(t, H, W):
  """tile -> (image, row, x0, x_new): conv32_lds.hip's tile_coords"""
  row, s = divmod(t, tiles_per_row(W))
  x_new = SEG * s
  return row // H, row % H, min(x_new, W - SEG), x_new


def conv32_lds_grid(B, H, W):
  return min(-(-ntiles(B, H, W) // 8) * 8, MAX_WG)


def wgrad_lds2(B, H, W):
  return ntiles(B, H, W) >= LDS2_TILES


def conv32_wgrad_lds_slabs(B, H, W):
  if wgrad_lds2(B, H, W):
    return 256
  return min(-(-(-(-ntiles(B, H, W) // 16)) // 8) * 8, 512)


def band(nt):
  return -(-nt // 8)


def wg_tiles(b, nt, grid, mut=None):
  """the tiles workgroup b walks, in its order"""
  t0 = (b & 7) * band(nt)
  t1 = min(t0 + band(nt) + (1 if mut == "band_off_1" else 0), nt)
  return range(t0 + (b >> 3), t1, grid // 8)


def wg_of_tile(t, nt, grid):
  """the workgroup that walks tile t (an int or an int64 tensor)"""
  xcd = t // band(nt)
  return ((t - xcd * band(nt)) % (grid // 8)) * 8 + xcd


def most_tiles(nt, grid):
  return max(len(wg_tiles(b, nt, grid)) for b in range(grid))


def owner_map(B, H, W, grid, device="cpu"):
  """[B, H, W] int64: the workgroup whose moments / next sums count each pixel — the tile of its 128-column segment: the
  duplicated columns of a shifted tile stay with the neighbour"""
  rows = torch.arange(B * H, device=device).view(B, H, 1)
  seg = (torch.arange(W, device=device) // SEG).view(1, 1, W)
  return wg_of_tile(rows * tiles_per_row(W) + seg, ntiles(B, H, W), grid)


def owner_map_loop(B, H, W, grid, mut=None):
  """the same by walking the tiles of every workgroup as the kernel does: (own [B, H, W] (-1: nobody), cover [B, H, W]: how many
  times each pixel is counted, cnt [grid])"""
  own = torch.full((B, H, W), -1, dtype=torch.int64)
  cover = torch.zeros(B, H, W, dtype=torch.int64)
  cnt = torch.zeros(grid, dtype=torch.int64)
  nt = ntiles(B, H, W)
  for b in range(grid):
    for t in wg_tiles(b, nt, grid, mut):
      i, y, x0, x_new = tile_coords(t, H, W)
      dup = x_new - x0
      if mut == "dup_twice":
        dup = 0
      elif mut == "dup_off_1" and dup > 0:
        dup += 1
      for wave in range(4):                      # the kernel's three cases per wave
        d_w = dup - 32 * wave
        lo = x0 + 32 * wave + (0 if d_w <= 0 else min(d_w, 32))
        hi = x0 + 32 * wave + 32
        own[i, y, lo:hi] = b
        cover[i, y, lo:hi] += 1
        cnt[b] += hi - lo
  return own, cover, cnt


def flat_owner(B, H, W, per, device="cpu"):
  """partials of the kernels below W = 128: `per` consecutive voxels of the flattened interior each"""
  return (torch.arange(B * H * W, device=device) // per).view(B, H, W)


# ----------------------------------------------------------------------------- routes (csrc/conv_entry.hip, for 3x3 stride 1)
def lds_applicable(W, d, hin):
  return 1 <= d <= 8 and hin[1] >= 8 and hin[0] >= d and W >= SEG


def fwd_route(B, H, W, d, hin):
  if lds_applicable(W, d, hin):
    return "lds2d"
  return "splitk" if B * H * W <= SPLITK_MAX_M else "direct"


def stat_parts(B, H, W, d, hin):
  r = fwd_route(B, H, W, d, hin)
  return conv32_lds_grid(B, H, W) if r == "lds2d" else -(-B * H * W // (32 if r == "splitk" else 128))


def bnbwd_parts(B, H, W, d, hin):
  return conv32_lds_grid(B, H, W) if lds_applicable(W, d, hin) else 0


def wgrad_route(B, H, W, d, hin, hout):
  if lds_applicable(W, d, hin) and hout[1] >= 8:
    return "lds2" if wgrad_lds2(B, H, W) else "lds"
  return "generic"


def wgrad_workspace(B, H, W, d, hin, hout):
  """floats; None on the generic route (its plan is not restated here: the slab count is the library's)"""
  if wgrad_route(B, H, W, d, hin, hout) == "generic":
    return None
  return conv32_wgrad_lds_slabs(B, H, W) * (9 * 1024 + 32)


def wgrad_bnapply_ok(B, H, W, d, hin, hout):
  return 1 if wgrad_route(B, H, W, d, hin, hout) == "lds2" else 0


# ----------------------------------------------------------------------------- the launches restated tile by tile
def conv_tiles(x, w, d, dtype=F64, transposed=False, mut=None):
  """the convolution as the kernel walks it: per segment the three staged rows y - d, y, y + d over the columns x0 - 8 ..
  x0 + 135 (zero outside the image), nine taps at column 8 + v + (kx - 1) d; a shifted segment overwrites its duplicates"""
  B, H, W, _ = x.shape
  we = wr._eff(w, transposed, dtype).to(x.device)
  xp = F.pad(x.to(dtype), (0, 0, 8, 8, d, d))
  out = torch.full((B, H, W, we.shape[0]), float("nan"), dtype=dtype, device=x.device)
  for s in range(tiles_per_row(W)):
    x0 = min(SEG * s, W - SEG)
    acc = torch.zeros(B, H, SEG, we.shape[0], dtype=dtype, device=x.device)
    for ky in range(3):
      staged = xp[:, ky * d:ky * d + H, x0:x0 + SEG + 16]
      for kx in range(3):
        if mut == "drop_tap" and (ky, kx) == (1, 2):               # (a centre-row tap: inside the image at every H)
          continue
        off = 8 + (kx - 1) * (d - 1 if mut == "tap_dm1" else d)
        acc += torch.matmul(staged[:, :, off:off + SEG], we[:, :, ky, kx].t())
    out[:, :, x0:x0 + SEG] = acc
  return out


def eval_tiles(x, w, bias, scale, shift, slope, res, d, mut=None):
  """epilogue 1: lrelu(z scale + shift) (+ residual); res "self": the staged centre row (conv32_lds_skip_kernel)"""
  slope = f32(slope)
  y = (conv_tiles(x, w, d) + wr._c(bias).to(x.device)) * wr._c(scale).to(x.device) + wr._c(shift).to(x.device)
  if isinstance(res, str):
    r = F.pad(x.double(), (0, 0, 0, 0, d, d))[:, :x.shape[1]] if mut == "skip_row" else x.double()
  else:
    r = res.double() if res is not None else None
  if mut == "res_before_act" and r is not None:
    y = y + r
    return torch.maximum(y, y * slope)
  out = torch.maximum(y, y * slope)
  return out + r if r is not None else out


def wgrad_tiles(x, gz, d, dtype=F64, mut=None):
  """the weight gradient as the kernels walk it: unshifted 128-column segments, g_z beyond W zero (mutant: what lies there in
  the unpadded flat image), x from the staged rows"""
  B, H, W, C = x.shape
  Wt = SEG * tiles_per_row(W)
  xp = F.pad(x.to(dtype), (0, 0, 8, Wt - W + 8, d, d))
  if mut == "g_wrapped":
    flat = F.pad(gz.to(dtype).reshape(B, H * W, C), (0, 0, 0, Wt))
    idx = torch.arange(H, device=x.device).view(H, 1) * W + torch.arange(Wt, device=x.device).view(1, Wt)
    ge = flat[:, idx.reshape(-1)].reshape(B, H, Wt, C)
  else:
    ge = F.pad(gz.to(dtype), (0, 0, 0, Wt - W))
  dW = torch.zeros(C, C, 3, 3, dtype=dtype, device=x.device)
  for s in range(tiles_per_row(W)):
    g = ge[:, :, SEG * s:SEG * s + SEG].reshape(-1, C)
    for ky in range(3):
      for kx in range(3):
        c0 = SEG * s + 8 + (kx - 1) * d
        dW[:, :, ky, kx] += torch.matmul(g.t(), xp[:, ky * d:ky * d + H, c0:c0 + SEG].reshape(-1, C))
  return dW, ge.reshape(-1, C).sum(0)


# ----------------------------------------------------------------------------- reference + bound of each launch
def forward_z(x32, w, bias, d, residual=None, transposed=False):
  """z = conv(x) + bias (+ residual) in float64 from the fp32 operands, and gamma(288 + r) S"""
  dev = x32.device
  z = conv_direct(x32, w, d, transposed=transposed)
  S = conv_direct(x32.abs(), w.abs(), d, transposed=transposed)
  if bias is not None:
    z, S = z + wr._c(bias).to(dev), S + wr._c(bias).abs().to(dev)
  n = N_K
  if residual is not None:
    z, S, n = z + residual.double(), S + residual.double().abs(), n + 1
  return dict(z=z, e_z=gamma(n) * S, S=S)


def eval_out(x32, w, bias, scale, shift, slope, residual, d):
  """epilogue 1 and gamma(288 + 3 + r) (|scale| S + |shift| + |residual|)"""
  dev, slope = x32.device, f32(slope)
  f = forward_z(x32, w, bias, d)
  y = f["z"] * wr._c(scale).to(dev) + wr._c(shift).to(dev)
  out = torch.maximum(y, y * slope)
  S = f["S"] * wr._c(scale).abs().to(dev) + wr._c(shift).abs().to(dev)
  n = N_K + 3
  if residual is not None:
    out, S, n = out + residual.double(), S + residual.double().abs(), n + 1
  return dict(out=out, e_out=gamma(n) * S)


def moments(z32, own, grid, n_lane):
  """(count [grid], mean, M2 [grid][32]) of workgroup k's owned pixels of the launch's own fp32 z: wino_ref.moments' lane model
  (shifted per-lane sums of n_lane values, an 8-way Chan merge) over this family's owner map"""
  z = z32.double()
  one = torch.ones(z.shape[:3] + (1,), dtype=F64, device=z.device)
  cnt = wr._scatter(one, own, grid)[:, 0]
  n = cnt.clamp(min=1).view(-1, 1)
  mean = wr._scatter(z, own, grid) / n
  dev = z - mean[own]
  m2 = wr._scatter(dev ** 2, own, grid)
  R = wr._scatter_max(dev.abs(), own, grid)
  e_lane = gamma(n_lane + 1) * 2 * R + U * mean.abs()
  e_mean = gamma(n_lane + 30) * 2 * R + 9 * U * mean.abs()
  e_m2 = 4 * gamma(3 * n_lane + 56) * n * R * R + 8 * R * e_lane * n
  return dict(cnt=cnt, mean=mean, m2=m2, e_mean=e_mean, e_m2=e_m2)


def moments_two_pass(z32, own, parts):
  """flat partials of conv_epilogue (conv32_mfma.hip): mean = sum / n, M2 = sum (z - mean)^2, each 16 per lane, the half
  merge, 3 wave adds"""
  z = z32.double()
  one = torch.ones(z.shape[:3] + (1,), dtype=F64, device=z.device)
  cnt = wr._scatter(one, own, parts)[:, 0]
  n = cnt.clamp(min=1).view(-1, 1)
  mean = wr._scatter(z, own, parts) / n
  m2 = wr._scatter((z - mean[own]) ** 2, own, parts)
  e_mean = gamma(21) * wr._scatter(z.abs(), own, parts) / n
  e_m2 = gamma(26) * (m2 + n * e_mean ** 2) + n * e_mean ** 2
  return dict(cnt=cnt, mean=mean, m2=m2, e_mean=e_mean, e_m2=e_m2)


def next_sums(gx32, z_next, n_scale, n_shift, n_mean, slope, own, grid, n_lane):
  """[grid][64]: sum g_y and sum g_y (z_next - mean) over workgroup k's owned pixels of the launch's own fp32 g_x
  (wino_ref.next_sums' model over this family's owner map), and the count of elements undecided on y_next"""
  dev, slope = gx32.device, f32(slope)
  gx, zn = gx32.double(), z_next.double()
  zs = zn * wr._c(n_scale).to(dev)
  y = zs + wr._c(n_shift).to(dev)
  und = y.abs() <= U * (1 + 2 * U) * (zs.abs() + y.abs())
  gy = torch.where(y > 0, gx, gx * slope)
  dm = zn - wr._c(n_mean).to(dev)
  slack = torch.where(und, gx.abs() * (1 - slope), torch.zeros_like(gx))
  sc = lambda v: wr._scatter(v, own, grid)
  sums = torch.cat([sc(gy), sc(gy * dm)], 1)
  e = torch.cat([gamma(n_lane + 2) * sc(gy.abs()) + sc(slack), gamma(n_lane + 3) * sc((gy * dm).abs()) + sc(slack * dm.abs())], 1)
  return dict(sums=sums, e_sums=e, undecided=int(und.sum()))


def undecided_next(z_next, n_scale, n_shift):
  zs = z_next.double() * wr._c(n_scale).to(z_next.device)
  y = zs + wr._c(n_shift).to(z_next.device)
  return int((y.abs() <= U * (1 + 2 * U) * (zs.abs() + y.abs())).sum())


def wgrad_roundings(route, B, H, W, slabs, accumulate):
  """(n of dW, n of db): see BOUNDS"""
  a = 1 if accumulate else 0
  if route == "generic":
    return B * H * W + 1 + a, B * H * W + 1 + a
  mt = most_tiles(ntiles(B, H, W), slabs)
  n_r = -(-slabs // 16) + 16
  if route == "lds":
    return 32 * mt + 3 + n_r + a, 16 * mt + 1 + 3 + n_r + a
  return 16 * mt + 7 + n_r + a, 8 * mt + 1 + 7 + n_r + a


def weight_gradient(x, gz32, d, route, slabs, dW0=None, db0=None):
  """dW, db in float64 from the fp32 operands and gamma(n) S_w"""
  B, H, W, _ = x.shape
  dW, db = wgrad_direct(x, gz32, d)
  SW, Sb = wgrad_direct(x.abs(), gz32.abs(), d)
  if dW0 is not None:
    dW, db, SW, Sb = dW + dW0.double().to(x.device), db + db0.double().to(x.device), SW + dW0.double().abs().to(x.device), \
        Sb + db0.double().abs().to(x.device)
  nW, nb = wgrad_roundings(route, B, H, W, slabs, dW0 is not None)
  return dict(dW=dW, db=db, e_dW=gamma(nW) * SW, e_db=gamma(nb) * Sb)


def exact_headroom(*abs_sums):
  """largest sum|terms| of the given absolute-value evaluations in quarter units (the exact family's quantum): a case is exact in
  fp32 while this stays below 2^24"""
  return 4.0 * max(float(s.max()) for s in abs_sums)


# ----------------------------------------------------------------------------- the cases
HALO_W = 8


def _c4(geom, d, hin=None, hout=None):
  hin = hin or (d, HALO_W)
  return (tuple(geom), d, tuple(hin), tuple(hout or hin))


def forward_cases():
  """(geometry, dilation, input halo (ph, pw), output halo) of every forward / weight-gradient case on the LDS kernels"""
  out = []
  for g in ((1, 3, 128), (1, 5, 129), (1, 9, 160)):
    out += [_c4(g, d) for d in (1, 2, 4, 8)]
  out += [_c4((1, 5, 129), 3), _c4((1, 5, 129), 7), _c4((2, 7, 255), 1), _c4((1, 6, 256), 2), _c4((1, 2, 257), 4),
          _c4((3, 29, 770), 3), _c4((3, 29, 770), 7),
          _c4((1, 9, 160), 2, (8, 12)),                      # a halo larger than the least accepted
          _c4((1, 5, 129), 1, (1, 8), (3, 9))]               # the output's halo differs from the input's
  return out


EXACT_CASES = [c for c in forward_cases() if c[2] == c[3]]    # (the exact family also runs residual == x: equal halos)
WGRAD_LARGE = [_c4((1, 3071, 128), 1), _c4((3, 1024, 128), 2), _c4((4, 384, 129), 4)]
WGRAD_NARROW_HALO = _c4((1, 5, 129), 1, (1, 8), (1, 7))      # output pw < 8: the generic weight gradient
BELOW_128 = [_c4((1, 9, 127), 2), _c4((3, 100, 127), 1)]     # split-K (M <= 32768), the direct kernel


def case_id(c):
  g, d, hin, hout = c
  return "%s-d%d" % (geom_id(g), d) + ("" if (hin, hout) == ((d, HALO_W), (d, HALO_W)) else "-in%dx%d-out%dx%d" % (hin + hout))
