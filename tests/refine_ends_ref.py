"""A plain float64 restatement of ONE launch each of the two ends of the edge-aware refinement — the 4 -> 32 input layer
(csrc/conv4_mfma.hip: as_pack_in4, as_conv4_fwd on staged rows and on one tile, as_conv4_wgrad, as_conv4_wgrad_bnapply,
as_conv4_wgrad_bnapply_proj, as_tap_gather) and the 32 -> 1 output layer (csrc/refine_out.hip: as_refine_out_fwd;
csrc/softargmax.hip, the thin 2-D path: as_conv32to1_fwd, as_conv32to1_bwd, as_conv32to1_dgrad_bnsums) with the glue between
them (csrc/optim.hip: as_relu_bwd, as_mirror_taps_ch0) — with the kernels' tiling restated as plain functions, the bound of
every output, and the cases tests/test_gpu_refine_ends_fp64.py runs.  CPU only as far as the library goes: nothing here imports
it; every function works on the device of its operands, so the GPU file runs the same code in float64 on the card.
tests/test_refine_ends_ref_cpu.py holds the restatements to torch's float64 convolutions and autograd, brackets an fp32 emulation
of each sum with its bound and shows that the cases tell the MUTANTS from the right restatement.

Tensors are channel-last interiors: maps [B, H, W, 32], the packed input x4 [B, H, W, 4], one-channel maps [B, H, W]; the input
layer's weight is torch's [32][4][3][3], the output layer's w [32][9] = conv2d_out.weight[0] with the taps flattened (t = 3 ky +
kx).  fp32 operands are taken as they are and widened.

TILING
  as_conv4_fwd     staged rows when W >= 32, both halos >= 1 and W + 2 pw >= 64 (a 64-pixel DMA window fits a padded row): a tile
                   is 32 consecutive columns of one row, the last tile of a row shifted left to end at W; its three input rows
                   come as 64-pixel windows starting at the padded column ps = xw - 1 + pw, clamped to pc = min(ps, Wp - 64)
                   with the LDS destination shifted by ps - pc; workgroups = min(ceil(tiles / 4), 1024), wave w of workgroup k
                   takes the tiles 4 k + w, + 4 grid, ..  Otherwise one tile of 128 voxels per workgroup.
  as_refine_out    a workgroup walks down a strip of RO_COLS = 126 columns and 32 (activation fused) or 12 (plain) rows; rows
                   ya - 1 .. yb are staged (128 voxels, one either side) and projected onto the nine taps into a ring of three
                   rows, slot (row + 1) % 3; everything outside the image is SELECTED as zero (no halo value is used)
  thin forward     patches of 16 x 32 staged voxels, 14 x 30 outputs; halo row / column -1, H, W of the tensor are READ
  thin backward    chunks of 128 voxels of one row: chunk ch = (b H + y) ceil(W / 128) + x / 128; workgroup k of `grid` takes
                   ch = k, k + grid, ..; grid = min(chunks, 16384) (data gradient), min(ceil(chunks / 4), 1024) (weight
                   gradient, and the 4 -> 32 layer's), min(chunks, 1024) (as_conv32to1_dgrad_bnsums: one fp64 slab [64] each)

BOUNDS, the project's rule, derived and never tuned (u = 2^-24, gamma(n) = n u / (1 - n u)): a sum of n terms added in ANY order
in fp32 errs by at most gamma(n) sum|terms|, sum|terms| the same operation on absolute values.  Where a launch consumes an fp32
tensor that it also wrote, or was handed, the sum is taken from that fp32 tensor widened.
  x4, mirrored taps, g_pre     bit-exact
  conv4 z (epilogue 0 / 2)     gamma(37) S: 36 products + the bias
  conv4 epilogue 1             gamma(40) (S |scale| + |shift|): + the product by scale, the shift, the slope (wino_ref.eval_out)
  a_out                        wino_ref.act_chain
  32 -> 1 out (all forms)      gamma(288 + 1 per given bias and add_src) (sum |a| |w| + |bias| + |add_src|), from the a the launch
                               wrote (fused) or was handed; the ReLU is 1-Lipschitz
  32 -> 1 g_a                  gamma(9) sum |g_out| |w|
  32 -> 1 g_w, g_bias          gamma(B H W (+ 1 with accumulate)) (sum |a| |g_out| (+ |value there|))
  bnsums slab k                per-lane fp32 sums of n_l = 4 * the most chunks of a workgroup terms, then an exact double sum:
                               gamma(n_l + 2) sum|g_y|, gamma(n_l + 3) sum|g_y| |z - mean| over the chunks of workgroup k, from
                               the launch's own fp32 g_a, + (1 - slope) |g_a| (|z - mean|) of every element undecided on y
  conv4 dW, db                 gamma(B H W (+ 1)) (sum |x| |g_z| (+ |value there|)) from the fp32 g_z given / written
  bnapply g_z                  wino_ref.gz_chain / judge_gz
  proj h                       gamma(32) sum |w_proj| |g_z| + sum |w_proj| e_gz; a pixel with an undecided channel is judged
                               against the nearer of the two branches
  proj dW, db                  from the float64 g_z chain: gamma(n) S + sum |x| e_gz, undecided elements entering both ways
                               (+ |x| |g_z(pos) - g_z(neg)|)
  tap gather                   gamma(9 + 1 with a residual) (sum |h| + |residual|)

EXACT CASES.  Small-integer data, nine single-tap weights and a dense one, scale 1, shift 0, slope 1/2, k1 = k2 = 0, k3 = 1: every
sum is exact in fp32 and must equal float64 bit for bit; headroom() is the largest sum|terms| in units of the quantum.

The sum functions take a dtype and a `mut`: float64 is the restatement, float32 the emulation in the kernels' tap order; a `mut`
is a deliberately WRONG restatement (MUTANTS), each a mistake an index path of these kernels could make.  A voxel a mutant never
writes is NaN; words it writes outside the interior are counted (`stray`)."""
import torch
import torch.nn.functional as F

import bn_ref as br
from trunk_ref import U, gamma_n
from wino_ref import act_chain, gz_chain, judge_gz, f32, ratio    # noqa: F401

F64 = torch.float64
NAN = float("nan")
RO_COLS, RO_ROWS_ACT, RO_ROWS_PLAIN = 126, 32, 12
TC_OR, TC_OC = 14, 30
CHUNK = 128
DGRAD_CAP, SLAB_CAP = 16384, 1024
C4_TILE, C4_CAP, C4_WINDOW = 32, 1024, 64
N_CONV4, N_CONV4_EP1, N_OUT, N_DGRAD, N_PROJ, N_GATHER = 37, 40, 288, 9, 32, 9

MUTANTS = {
    "ro_seam128": "refine_out: the column seam at 128 instead of 126 (the strips' first columns 128 apart)",
    "ro_ring_slot": "refine_out: the gather reads ring slot (yo + ky + 1) % 3",
    "ro_no_yb": "refine_out: the strip's last extra row yb is not staged (its projections read as zero)",
    "c4_end_Wm1": "conv4 rows: the last row segment shifted to end at W - 1",
    "c4_no_clamp_shift": "conv4 rows: the DMA window's clamp shift ps - pc not applied to the LDS destination",
    "tf_seam16": "thin forward: patch seams at 16 / 32 instead of 14 / 30",
    "tf_halo_zero": "thin forward: halo row H / halo column W read as zero when they hold data",
    "tb_not_mirrored": "thin backward: taps not mirrored",
    "tb_col_m1_zero": "thin backward: gradient-map column x0 - 1 of a chunk read as zero",
    "tb_ragged128": "thin backward: the ragged last chunk taken as 128 wide (g_a written beyond the row's end)",
    "bs_contiguous": "bnsums: a workgroup owns a contiguous block of chunks instead of every grid-th",
    "pj_not_mirrored": "proj: w_proj[t] = w[:, 0, t] instead of w[:, 0, 8 - t]",
    "tg_wrapped": "tap gather: a tap left / right of the image wraps into the neighbouring row instead of reading zero",
}
# as_refine_out's own-column mask taken as v <= 127 is NOT in the list: staged voxel 127 of a strip is column x0 + 126, which the
# mask's xx < W keeps inside the image, where the next strip writes the same element-wise value: no output word changes
# (tests/test_refine_ends_ref_cpu.py shows it with ro_a_out_writes).


def _v(t, dtype=F64):
  return t.to(dtype).view(1, 1, 1, -1)


def cdiv(a, b):
  return -(-a // b)


# ----------------------------------------------------------------------------- the small bit-exact launches
def pack_in4(ch0, img):
  """x4[b, y, x, :] = (ch0[b, y, x] if given), img[b, 0 .. C - 1, y, x], zeros up to four channels; img is [B, C, H, W]"""
  B, C, H, W = img.shape
  parts = ([ch0.reshape(B, H, W, 1)] if ch0 is not None else []) + [img.permute(0, 2, 3, 1)]
  x = torch.cat(parts, 3)
  return F.pad(x, (0, 4 - x.shape[3]))


def mirror_taps_ch0(w):
  """(by_tap [9][32], by_channel [32][9]) of w [32][Cin][3][3]: by_tap[t][c] = by_channel[c][t] = w[c][0][8 - t]"""
  m = w[:, 0].reshape(32, 9).flip(1)
  return m.t().contiguous(), m.contiguous()


def relu_bwd(g_out, out):
  """g_out where out > 0, else +0 (out == 0 and out == -0.0 give 0)"""
  return torch.where(out > 0, g_out, torch.zeros_like(g_out))


# ----------------------------------------------------------------------------- the 4 -> 32 layer, forward
def conv4_rows_route(W, ph, pw):
  return W >= C4_TILE and ph >= 1 and pw >= 1 and W + 2 * pw >= C4_WINDOW


def conv4_tiles(B, H, W):
  """(tiles, workgroups, waves that own no tile) of the staged-row route"""
  n = B * H * cdiv(W, C4_TILE)
  grid = min(cdiv(n, 4), C4_CAP)
  return n, grid, max(4 * grid - n, 0)


def conv4_stat_parts(B, H, W, ph, pw):
  return conv4_tiles(B, H, W)[1] if conv4_rows_route(W, ph, pw) else cdiv(B * H * W, 128)


def conv4_sum(x4, w, bias, dtype=F64, mut=None, pw=1):
  """z[b, y, x, co] = bias[co] + sum_{ky, kx, c} x4[b, y + ky - 1, x + kx - 1, c] w[co][c][ky][kx], x4 zero outside the image (it
  sits in a zero halo of pw columns), tile by tile as conv4_rows_kernel: the accumulator starts at the bias and takes the taps
  in order.  On the one-tile route the mutants do not apply."""
  B, H, W, _ = x4.shape
  dev = x4.device
  w, z0 = w.to(dtype).to(dev), (bias.to(dtype).to(dev) if bias is not None else torch.zeros(32, dtype=dtype, device=dev))
  rows = conv4_rows_route(W, 1, pw)
  Wp = W + 2 * pw
  xp = F.pad(x4.to(dtype), (0, 0, pw, pw, 1, 1))                 # [B, H + 2, Wp, 4]
  z = torch.full((B, H, W, 32), NAN, dtype=dtype, device=dev)
  tiles = [min(C4_TILE * j, W - C4_TILE) for j in range(cdiv(W, C4_TILE))] if rows else [0]
  width = C4_TILE if rows else W
  for j, xw in enumerate(tiles):
    if mut == "c4_end_Wm1" and C4_TILE * j >= W - C4_TILE:
      xw = W - C4_TILE - 1
    ps = xw - 1 + pw
    pc = min(ps, Wp - C4_WINDOW) if rows else ps
    first = pc if mut == "c4_no_clamp_shift" else ps            # the padded column that lands at slot C4_SLOT0
    acc = z0.view(1, 1, 1, 32).expand(B, H, width, 32)
    for ky in range(3):
      for kx in range(3):
        if bool(w[:, :, ky, kx].any()):
          acc = acc + torch.matmul(xp[:, ky:ky + H, first + kx:first + kx + width], w[:, :, ky, kx].t())
    z[:, :, xw:xw + width] = acc
  return z


def conv4_forward(x4, w, bias, scale=None, shift=None, slope=0.2):
  """z and gamma(37) S; with scale / shift epilogue 1: lrelu(z scale + shift) and gamma(40) (S |scale| + |shift|)"""
  dev = x4.device
  z = conv4_sum(x4, w, bias)
  S = conv4_sum(x4.abs(), w.abs(), bias.abs() if bias is not None else None)
  if scale is None:
    return dict(z=z, e_z=gamma_n(N_CONV4) * S, S=S)
  y = z * _v(scale).to(dev) + _v(shift).to(dev)
  return dict(z=torch.maximum(y, y * f32(slope)), e_z=gamma_n(N_CONV4_EP1) * (S * _v(scale).abs().to(dev) + _v(shift).abs().to(dev)))


# ----------------------------------------------------------------------------- the 32 -> 1 layer, forward
def _project(ae, w, dtype):
  """P[.., t] = sum_c a[.., c] w[c][t]: the channels one by one in order in fp32 (the matrix pipe's K order, the fmaf chain)"""
  w = w.to(dtype).to(ae.device)
  if dtype == F64:
    return torch.matmul(ae.to(dtype), w)
  P = torch.zeros(ae.shape[:-1] + (9,), dtype=dtype, device=ae.device)
  for c in range(32):
    P = P + ae[..., c:c + 1].to(dtype) * w[c].view(1, 1, 1, 9)
  return P


def conv_out_sum(a, w, bias=None, add_src=None, relu=0, dtype=F64, ring=None, row_of=None, drop=None):
  """out[b, y, x] = relu?(bias + sum_{ky, kx} P[b, y + ky - 1, x + kx - 1][3 ky + kx] + add_src): "project, then gather", the
  accumulator starting at the bias, the taps in order, add_src last.  ring: a [B, H + 2, W + 2, 32] whose border is what lies
  around the image (zeros when None).  row_of / drop: hooks of the mutants."""
  B, H, W, _ = a.shape
  ae = F.pad(a.to(dtype), (0, 0, 1, 1, 1, 1)) if ring is None else ring.to(dtype)
  P = _project(ae, w, dtype)
  out = (bias.to(dtype).to(a.device).reshape(1, 1, 1) if bias is not None else torch.zeros(1, 1, 1, dtype=dtype, device=a.device)).expand(B, H, W)
  for ky in range(3):
    r = ky if row_of is None else row_of(ky)
    for kx in range(3):
      term = P[:, r:r + H, kx:kx + W, 3 * ky + kx]
      if drop is not None and ky == 2:
        term = term * drop.to(dtype).view(1, H, 1)
      out = out + term
  if add_src is not None:
    out = out + add_src.to(dtype)
  return torch.clamp(out, min=0) if relu else out


def ro_rows(act):
  return RO_ROWS_ACT if act else RO_ROWS_PLAIN


def ro_grid(B, H, W, act):
  """(strips of columns, strips of rows, workgroups) of as_refine_out_fwd"""
  return cdiv(W, RO_COLS), cdiv(H, ro_rows(act)), B * cdiv(W, RO_COLS) * cdiv(H, ro_rows(act))


def refine_out_ok(D, pd, ph, pw, W):
  return D == 1 and pd == 0 and ph >= 1 and pw >= 1 and ph * (W + 2 * pw) >= 128


def refine_out_sum(a, w, bias=None, add_src=None, relu=0, act=True, dtype=F64, mut=None):
  """as_refine_out_fwd's out from the activated input a, strip by strip"""
  B, H, W, _ = a.shape
  rows = ro_rows(act)
  row_of, drop = None, None
  if mut == "ro_ring_slot":                                     # slot (yo + ky + 1) % 3 holds input row yo + (ky + 1) % 3 - 1
    row_of = lambda ky: (ky + 1) % 3
  if mut == "ro_no_yb":
    y = torch.arange(H, device=a.device)
    drop = ~(((y + 1) % rows == 0) & (y + 1 < H))
  out = conv_out_sum(a, w, bias, add_src, relu, dtype, row_of=row_of, drop=drop)
  if mut == "ro_seam128":                                       # strip seg writes the columns 128 seg .. 128 seg + 125
    x = torch.arange(W, device=a.device)
    out = torch.where((x % 128 < RO_COLS) & (x // 128 < cdiv(W, RO_COLS)), out, torch.full_like(out, NAN))
  return out


def ro_a_out_writes(W, own_last=RO_COLS):
  """how often as_refine_out_fwd writes each column of a_out, with the own-column mask 1 <= v <= own_last"""
  n = torch.zeros(W, dtype=torch.int64)
  for seg in range(cdiv(W, RO_COLS)):
    for v in range(1, own_last + 1):
      if seg * RO_COLS - 1 + v < W:
        n[seg * RO_COLS - 1 + v] += 1
  return n


def thin_fwd_sum(a, w, bias=None, add_src=None, relu=0, dtype=F64, mut=None, ring=None):
  """conv32to1_2d_fwd_kernel's out, patch by patch; ring as in conv_out_sum (the kernel reads the tensor's halo)"""
  B, H, W, _ = a.shape
  if mut == "tf_halo_zero" and ring is not None:
    ring = ring.clone()
    ring[:, H + 1] = 0
    ring[:, :, W + 1] = 0
  out = conv_out_sum(a, w, bias, add_src, relu, dtype, ring=ring)
  if mut == "tf_seam16":                                        # patch (ty, tx) writes rows 16 ty .. + 13, columns 32 tx .. + 29
    y, x = torch.arange(H, device=a.device), torch.arange(W, device=a.device)
    oky = (y % 16 < TC_OR) & (y // 16 < cdiv(H, TC_OR))
    okx = (x % 32 < TC_OC) & (x // 32 < cdiv(W, TC_OC))
    out = torch.where(oky.view(1, H, 1) & okx.view(1, 1, W), out, torch.full_like(out, NAN))
  return out


def out_layer(a32, w, bias, add_src, relu, ring=None):
  """out and gamma(288 + 1 per given bias and add_src) S from the fp32 a the launch wrote or was handed"""
  n = N_OUT + (bias is not None) + (add_src is not None)
  out = conv_out_sum(a32, w, bias, add_src, relu, ring=ring)
  S = conv_out_sum(a32.abs(), w.abs(), bias.abs() if bias is not None else None, add_src.abs() if add_src is not None else None, 0,
                   ring=ring.abs() if ring is not None else None)
  return dict(out=out, e_out=gamma_n(n) * S, S=S)


# ----------------------------------------------------------------------------- the 32 -> 1 layer, backward
def chunks(B, H, W):
  return cdiv(W, CHUNK), B * H * cdiv(W, CHUNK)


def dgrad_grid(B, H, W):
  return min(chunks(B, H, W)[1], DGRAD_CAP)


def wgrad_grid(B, H, W):
  return max(min(cdiv(chunks(B, H, W)[1], 4), SLAB_CAP), 1)


def bnsums_parts(B, H, W):
  return min(chunks(B, H, W)[1], SLAB_CAP)


def _taps_of(g, dtype, mut):
  """[9] maps G_t[b, y, x] = g_out[b, y + 1 - ky, x + 1 - kx] (zero outside the image): what tap t = 3 ky + kx of the backward
  kernels reads for voxel (y, x) from the three staged rows"""
  B, H, W = g.shape
  gp = F.pad(g.to(dtype), (1, 1, 1, 1))
  out = []
  for ky in range(3):
    for kx in range(3):
      s = gp[:, ky:ky + H, kx:kx + W] if mut == "tb_not_mirrored" else gp[:, 2 - ky:2 - ky + H, 2 - kx:2 - kx + W]
      if mut == "tb_col_m1_zero" and kx == 2:                   # sg[.][0] of a chunk: voxel x0 reading column x0 - 1
        x = torch.arange(W, device=g.device)
        s = s * (x % CHUNK != 0).to(dtype).view(1, 1, W)
      out.append(s)
  return out


def thin_dgrad_sum(g_out, w, dtype=F64, mut=None):
  """g_a[b, y, x, c] = sum_{ky, kx} g_out[b, y + 1 - ky, x + 1 - kx] w[c][3 ky + kx], the taps in order; and `stray`: the voxels
  written beyond a row's end (into the halo, or the next row)"""
  B, H, W = g_out.shape
  w = w.to(dtype).to(g_out.device)
  acc = torch.zeros(B, H, W, 32, dtype=dtype, device=g_out.device)
  for t, G in enumerate(_taps_of(g_out, dtype, mut)):
    acc = acc + G.unsqueeze(-1) * w[:, t].view(1, 1, 1, 32)
  stray = B * H * (cdiv(W, CHUNK) * CHUNK - W) if mut == "tb_ragged128" else 0
  return acc, stray


def data_gradient(g_out, w):
  g_a, _ = thin_dgrad_sum(g_out, w)
  S, _ = thin_dgrad_sum(g_out.abs(), w.abs())
  return dict(g_a=g_a, e_g_a=gamma_n(N_DGRAD) * S)


def thin_wgrad_sum(a, g_out, dtype=F64, mut=None):
  """g_w[c][t] = sum_{b, y, x} a[b, y, x, c] g_out[b, y + 1 - ky, x + 1 - kx],  g_bias = sum g_out"""
  B, H, W, C = a.shape
  am = a.to(dtype).reshape(-1, C)
  g_w = torch.stack([torch.matmul(G.reshape(1, -1), am)[0] for G in _taps_of(g_out, dtype, mut)], 1)
  return g_w, g_out.to(dtype).sum().reshape(1)


def weight_gradient(a, g_out, g_w0=None, g_b0=None):
  """g_w [32][9], g_bias [1] and gamma(B H W (+ 1)) S"""
  B, H, W, _ = a.shape
  g_w, g_b = thin_wgrad_sum(a, g_out)
  Sw, Sb = thin_wgrad_sum(a.abs(), g_out.abs())
  n = B * H * W
  if g_w0 is not None:
    g_w, g_b, Sw, Sb, n = g_w + g_w0.double(), g_b + g_b0.double(), Sw + g_w0.double().abs(), Sb + g_b0.double().abs(), n + 1
  return dict(g_w=g_w, g_b=g_b, e_g_w=gamma_n(n) * Sw, e_g_b=gamma_n(n) * Sb)


def chunk_owner(B, H, W, grid, mut=None, device="cpu"):
  """[B, H, W] int64: the workgroup whose loop ch = k, k + grid, .. reaches the voxel's chunk"""
  cpr, n = chunks(B, H, W)
  ch = (torch.arange(B * H, device=device).view(B, H, 1) * cpr + (torch.arange(W, device=device) // CHUNK).view(1, 1, W))
  if mut == "bs_contiguous":
    return ch // cdiv(n, grid)
  return ch % grid


def chunk_owner_loop(B, H, W, grid):
  """the same map by walking every workgroup's loop, as the kernels do (for the CPU test)"""
  cpr, n = chunks(B, H, W)
  own = torch.full((B * H, W), -1, dtype=torch.int64)
  for k in range(grid):
    for ch in range(k, n, grid):
      rowi, cx = divmod(ch, cpr)
      own[rowi, cx * CHUNK:min(cx * CHUNK + CHUNK, W)] = k
  return own.view(B, H, W)


def _slabs(v, own, grid):
  return torch.zeros(grid, v.shape[-1], dtype=F64, device=v.device).index_add_(0, own.reshape(-1), v.reshape(-1, v.shape[-1]))


def bn_sums(ga32, z, scale, shift, mean, slope, grid, mut=None):
  """[grid][64]: sum g_y and sum g_y (z - mean) over workgroup k's chunks of the launch's own fp32 g_a, with bounds, and the
  count of elements undecided on y = z scale + shift"""
  B, H, W, _ = ga32.shape
  dev, slope = ga32.device, f32(slope)
  ga, zz = ga32.double(), z.double()
  zs = zz * _v(scale).to(dev)
  y = zs + _v(shift).to(dev)
  und = y.abs() <= U * (1 + 2 * U) * (zs.abs() + y.abs())
  gy = torch.where(y > 0, ga, ga * slope)
  dm = zz - _v(mean).to(dev)
  slack = torch.where(und, ga.abs() * (1 - slope), torch.zeros_like(ga))
  own = chunk_owner(B, H, W, grid, mut, dev)
  sc = lambda v: _slabs(v, own, grid)
  nl = 4 * cdiv(chunks(B, H, W)[1], grid)
  sums = torch.cat([sc(gy), sc(gy * dm)], 1)
  e = torch.cat([gamma_n(nl + 2) * sc(gy.abs()) + sc(slack), gamma_n(nl + 3) * sc((gy * dm).abs()) + sc(slack * dm.abs())], 1)
  return dict(sums=sums, e_sums=e, undecided=int(und.sum()))


# ----------------------------------------------------------------------------- the 4 -> 32 layer, backward
def conv4_wgrad_sum(x4, gz, dtype=F64):
  """dW[co][c][ky][kx] = sum_{b, y, x} x4[b, y + ky - 1, x + kx - 1, c] g_z[b, y, x, co],  db[co] = sum g_z"""
  B, H, W, _ = x4.shape
  xp, g = F.pad(x4.to(dtype), (0, 0, 1, 1, 1, 1)), gz.to(dtype).reshape(-1, 32)
  dW = torch.zeros(32, 4, 3, 3, dtype=dtype, device=x4.device)
  for ky in range(3):
    for kx in range(3):
      dW[:, :, ky, kx] = torch.matmul(g.t(), xp[:, ky:ky + H, kx:kx + W].reshape(-1, 4))
  return dW, g.sum(0)


def conv4_weight_gradient(x4, gz32, dW0=None, db0=None, e_gz=None, both=None):
  """dW, db and gamma(B H W (+ 1)) S from the fp32 g_z given or written; for the proj launch (g_z never stored) gz32 is the
  float64 chain's g_z, e_gz its bound and `both` = |g_z(pos) - g_z(neg)| on the undecided elements: + sum |x| (e_gz + both)"""
  B, H, W, _ = x4.shape
  dW, db = conv4_wgrad_sum(x4, gz32)
  SW, Sb = conv4_wgrad_sum(x4.abs(), gz32.abs())
  n = B * H * W
  if dW0 is not None:
    dW, db, SW, Sb, n = dW + dW0.double(), db + db0.double(), SW + dW0.double().abs(), Sb + db0.double().abs(), n + 1
  e_dW, e_db = gamma_n(n) * SW, gamma_n(n) * Sb
  if e_gz is not None:
    pw, pb = conv4_wgrad_sum(x4.abs(), e_gz + (both if both is not None else 0.0))
    e_dW, e_db = e_dW + pw, e_db + pb
  return dict(dW=dW, db=db, e_dW=e_dW, e_db=e_db)


def gz_both(ref):
  """|g_z(pos) - g_z(neg)| where the branch is undecided, zero elsewhere"""
  return torch.where(ref["undecided"], (ref["pos"] - ref["neg"]).abs(), torch.zeros_like(ref["pos"]))


def gz_bound(ref):
  return torch.where(ref["positive"], ref["e_pos"], ref["e_neg"])


def proj_sum(gz, w, dtype=F64, mut=None):
  """h[b, t, y, x] = sum_co g_z[b, y, x, co] w_proj[t][co],  w_proj[t][co] = w[co][0][8 - t] (w the layer's [32][4][3][3])"""
  by_tap = mirror_taps_ch0(w)[0] if mut != "pj_not_mirrored" else w[:, 0].reshape(32, 9).t()
  return torch.matmul(gz.to(dtype), by_tap.to(dtype).to(gz.device).t()).permute(0, 3, 1, 2)


def proj_planes(ref, w):
  """h from gz_chain's result: the value on float64's branches, on all-positive / all-negative for the undecided elements, the
  bound gamma(32) sum |w_proj| |g_z| + sum |w_proj| e_gz, and the pixels with an undecided channel"""
  e = gamma_n(N_PROJ) * proj_sum(ref["g_z"].abs(), w.abs()) + proj_sum(gz_bound(ref), w.abs())
  alt = {k: proj_sum(torch.where(ref["undecided"], ref[k], ref["g_z"]), w) for k in ("pos", "neg")}
  return dict(h=proj_sum(ref["g_z"], w), h_pos=alt["pos"], h_neg=alt["neg"], e_h=e, undecided=ref["undecided"].any(-1))


def judge_h(got, p):
  g = got.double().reshape(p["h"].shape)
  r = lambda ref: ((g - ref).abs() / p["e_h"].clamp(min=1e-300))
  q = torch.where(p["undecided"].unsqueeze(1), torch.minimum(r(p["h_pos"]), r(p["h_neg"])), r(p["h"]))
  q = torch.where(g == p["h"], torch.zeros_like(q), q)
  return float(q.nan_to_num(float("inf")).max())


def tap_gather_sum(h, residual=None, dtype=F64, mut=None):
  """out[b, y, x] = residual[b, y, x] + sum_t h[b, t, y + t / 3 - 1, x + t % 3 - 1] (zero outside the image), the accumulator
  starting at the residual"""
  B, _, H, W = h.shape
  out = residual.to(dtype) if residual is not None else torch.zeros(B, H, W, dtype=dtype, device=h.device)
  if mut == "tg_wrapped":
    flat = F.pad(F.pad(h.to(dtype), (0, 0, 1, 1)).reshape(B, 9, -1), (1, 1))      # rows -1 and H zero, columns run on
    for t in range(9):
      o = 1 + (t // 3) * W + t % 3 - 1
      out = out + flat[:, t, o:o + H * W].reshape(B, H, W)
    return out
  hp = F.pad(h.to(dtype), (1, 1, 1, 1))
  for t in range(9):
    out = out + hp[:, t, t // 3:t // 3 + H, t % 3:t % 3 + W]
  return out


def tap_gather(h32, residual):
  out = tap_gather_sum(h32, residual)
  S = tap_gather_sum(h32.abs(), residual.abs() if residual is not None else None)
  return dict(out=out, e_out=gamma_n(N_GATHER + (residual is not None)) * S)


def g_up64(gz, w, g_pre):
  """the data gradient of the layer's disparity channel from g_z, in its direct form: g_pre + sum_{co, ky, kx} g_z[y + 1 - ky,
  x + 1 - kx, co] w[co][0][ky][kx]"""
  return conv_out_sum(gz, mirror_taps_ch0(w)[1], None, g_pre, 0)


# ----------------------------------------------------------------------------- BatchNorm coefficients of a case
def bn_coef(g_a, z, st, gamma, slope=0.2):
  """[96] (float64) = k1, k2, k3 of stage 3, from bn_ref.bn_bwd64 on the case's own data: g_z = (g_y - k1 - (z - mean) k2) k3"""
  r = br.bn_bwd64(g_a.cpu(), z.cpu(), {k: v.cpu() for k, v in st.items()}, gamma.cpu(), f32(slope))
  N = g_a.numel() // 32
  inv = st["invstd"].double().cpu()
  return torch.cat([r["sum_dy"] / N, inv * inv * r["sum_dx"] / N, gamma.double().cpu() * inv])


# ----------------------------------------------------------------------------- the cases
CONV4_ROWS = [(1, 1, 62), (2, 3, 62), (2, 5, 63), (2, 5, 64), (2, 5, 65), (1, 4, 95), (1, 4, 96), (1, 4, 97), (2, 7, 131),
              (1, 106, 1242)]
CONV4_ONE_TILE = [(2, 5, 61), (1, 1, 1), (2, 9, 31)]
CONV4_HALO2 = (2, 5, 65)                                        # the one case with the x4 halo (2, 2)
REFINE_OUT = [(2, H, W) for W in (1, 125, 126, 127, 253) for H in (1, 12, 13, 32, 33)]
REFINE_OUT_HALO1 = (2, 5, 126)                                  # halo (1, 1): the last staged row ends at the buffer's end
THIN_FWD = [(2, H, W) for W in (1, 30, 31, 61) for H in (1, 14, 15, 29)]
THIN_BWD = [(1, 1, 1), (1, 5, 100), (2, 3, 127), (2, 3, 128), (2, 3, 129), (1, 2, 257), (2, 2049, 3)]
THIN_BWD_DGRAD_CAP = (4, 4097, 2)                               # 16388 chunks: the data gradient's cap alone
BNSUMS = [(2, 3, 127), (2, 3, 128), (2, 3, 129), (3, 343, 5)]
CONV4_WGRAD = [(1, 1, 1), (1, 5, 100), (2, 3, 127), (2, 3, 128), (2, 3, 129), (1, 2, 257), (2, 2049, 3)]
CONV4_WGRAD_HALO2 = (2, 3, 129)                                 # the one case with the x4 halo (2, 2)
TAP_GATHER = [(2, H, W) for W in (1, 255, 256, 257) for H in (1, 2)]
RELU_BWD_N = (1, 3, 4, 1023, 1024, 1029)
EXACT_WEIGHTS = [("tap", t) for t in range(9)] + [("dense", 0)]


def geom_id(g):
  return "%dx%dx%d" % tuple(g)


def _gen(seed):
  return torch.Generator().manual_seed(seed)


def _seed(geom, k):
  B, H, W = geom
  return 100003 * k + 7 * B + 131 * H + W


def sentinels(t, val=1e4):
  """+-val ADDED on the first and last rows and columns of a [B, H, W, ..] map: the values stay distinct where a one- or
  two-row map is all border"""
  t[:, 0] += val; t[:, -1] -= val; t[:, :, 0] -= val; t[:, :, -1] += val
  return t


def state(seed, device="cpu"):
  """a BatchNorm state (mean, invstd, scale, shift) and its gamma"""
  g = _gen(seed)
  mean = torch.randn(32, generator=g) * 0.1
  invstd = torch.randn(32, generator=g).abs() + 0.5
  gamma = torch.randn(32, generator=g).abs() + 0.5
  scale = invstd * gamma
  shift = torch.randn(32, generator=g) * 0.1 - mean * scale
  return {k: v.to(device) for k, v in dict(mean=mean, invstd=invstd, scale=scale, shift=shift).items()}, gamma.to(device)


def case(geom, device="cpu"):
  """The random family of one geometry, fp32 on `device`: N(0, 1) maps with +-1e4 sentinels on the first and last rows and
  columns of every input (added: sentinels), weights N(0, 1) * 0.2."""
  B, H, W = geom
  T = lambda k, *s: torch.randn(B, H, W, *s, generator=_gen(_seed(geom, k))).to(device)      # (the same values on every device)
  c = {n: sentinels(T(k, 32)) for k, n in enumerate(("z", "skip", "a", "g_a"))}
  c.update({n: sentinels(T(10 + k)) for k, n in enumerate(("up", "g_out"))})
  c["x4"] = sentinels(T(20, 4))
  c["out"] = T(21)                                              # (the final ReLU's output, for as_relu_bwd: mixed signs)
  g = _gen(_seed(geom, 30))
  c["w_out"] = (torch.randn(32, 9, generator=g) * 0.2).to(device)
  c["b_out"] = (torch.randn(1, generator=g) * 0.1).to(device)
  c["w_in"] = (torch.randn(32, 4, 3, 3, generator=g) * 0.2).to(device)
  c["b_in"] = (torch.randn(32, generator=g) * 0.1).to(device)
  c["g_w0"], c["g_b0"] = torch.randn(32, 9, generator=g).to(device), torch.randn(1, generator=g).to(device)
  c["dW0"], c["db0"] = torch.randn(32, 4, 3, 3, generator=g).to(device), torch.randn(32, generator=g).to(device)
  c["st"], c["gamma"] = state(_seed(geom, 31), device)
  c["slope"] = 0.2
  return c


def _ints(shape, seed, device, lo=-2, hi=2):
  return torch.randint(lo, hi + 1, shape, generator=_gen(seed)).float().to(device)


def exact_case(geom, wfam, device="cpu"):
  """The integer family: maps in {-2 .. 2}, slope 1/2, scale 1, shift 0, mean 0, k1 = k2 = 0, k3 = 1; wfam ("tap", t): only tap
  t of both weights is non-zero (integers in {-2 .. 2}); ("dense", 0): all nine."""
  B, H, W = geom
  c = {n: _ints((B, H, W, 32), _seed(geom, 40 + k), device) for k, n in enumerate(("z", "skip", "a", "g_a"))}
  c.update({n: _ints((B, H, W), _seed(geom, 50 + k), device) for k, n in enumerate(("up", "g_out"))})
  c["x4"] = _ints((B, H, W, 4), _seed(geom, 60), device)
  g = _gen(_seed(geom, 61) + 31 * wfam[1])
  w_out = torch.randint(-2, 3, (32, 9), generator=g).float()
  w_in = torch.randint(-2, 3, (32, 4, 3, 3), generator=g).float()
  if wfam[0] == "tap":
    keep = torch.zeros(9)
    keep[wfam[1]] = 1
    w_out, w_in = w_out * keep, w_in * keep.view(1, 1, 3, 3)
  c["w_out"], c["w_in"] = w_out.to(device), w_in.to(device)
  c["b_out"], c["b_in"] = torch.tensor([3.0], device=device), torch.randint(-2, 3, (32,), generator=g).float().to(device)
  c["g_w0"], c["g_b0"] = torch.randint(-8, 9, (32, 9), generator=g).float().to(device), torch.tensor([-5.0], device=device)
  c["dW0"], c["db0"] = torch.randint(-8, 9, (32, 4, 3, 3), generator=g).float().to(device), torch.randint(-8, 9, (32,), generator=g).float().to(device)
  one, zero = torch.ones(32, device=device), torch.zeros(32, device=device)
  c["st"], c["gamma"] = dict(mean=zero, invstd=one, scale=one, shift=zero), one
  c["coef"] = torch.cat([zero, zero, one])
  c["slope"] = 0.5
  return c


def headroom(*sums):
  """the largest sum|terms| of the given absolute-value sums, in units of the quantum 1/4 (integers times halves of integers):
  an exact case needs it below 2^24"""
  return max(float(s.max()) for s in sums) / 0.25
