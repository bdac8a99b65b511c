"""A plain float64 restatement of ONE launch each of the minimal-filtering kernels of the edge-aware refinement's six dilated
32 -> 32 layers (csrc/conv32_wino.hip, conv32_wino_dgrad.hip + conv32_wino_dgrad_role.h, conv32_wino_wgrad.hip,
conv32_wino_bwd.hip): as_conv32_wino_pack_weights (used through the convolutions), as_conv32_wino_fwd, as_conv32_wino_eval,
as_conv32_wino_bwd_data, as_conv32_wino_bwd_filter and as_conv32_wino_bwd_fused — with the kernels' tiling restated as plain
functions of (B, H, W, d, grid), the bound of every output, and the cases tests/test_gpu_wino_fp64.py runs.  CPU only as far
as the library goes: nothing here imports it; every function works on the device of its operands, so the GPU file may run
the same code in float64 on the card.  tests/test_wino_ref_cpu.py holds the restatements to torch's float64 convolutions,
brackets the fp32 emulation with the bounds and shows that the cases tell the MUTANTS from the right restatement.

Tensors are channel-last interiors [B, H, W, 32], weights torch's [co][ci][3][3]; fp32 operands are taken as they are and
widened.  The convolution of a launch is always taken from the fp32 operand the launch itself produced (a_out for z, g_z for
g_x and dW), read back: the element-wise chain and the convolution are judged separately.

TILING (conv32_wino_kernel's order; the same loop heads every kernel of the family)
  a unit is (image, 64-column segment, comb r0 of rows r0, r0 + d, .., pair of comb rows): pairs(H, d) units per (image,
  segment), units = B ceil(W / 64) pairs; workgroup k of `grid` owns units [units k // grid, units (k + 1) // grid); a unit
  number decodes as ((image, segment), comb by comb, pair).  Segment seg starts at min(64 seg, W - 64): the last one is shifted
  back to end at the image edge and owns all its 64 columns, its neighbour (the last but one of a ragged row) keeps its first
  W - 64 (nseg - 1).  Tile t of a segment covers the columns c0(t), c0(t) + d, c0(t) = ((t >> L) << (L + 1)) | (t & (d - 1)),
  its input tile the columns c0 - d .. c0 + 2d and the comb rows j - 1 .. j + 2 of the pair (j, j + 1); rows and columns
  outside the image are zero.  Partition rules that differ: the stand-alone weight gradient (conv32_wino_wgrad.hip) does NOT
  shift the last segment (x0 = 64 seg, g_z beyond the image edge reads as zero): `shifted=False`; the fused backward's
  weight-gradient waves use the forward's segments and read the neighbour's unowned g_z columns as zero: `shifted=True`.
  grid: 512 (forward, data gradient), 256 (weight gradient slabs, fused backward).

BOUNDS, derived and counted from the code, never fitted (u = 2^-24, gamma(n) = n u / (1 - n u); a sum of n terms added in any
order in fp32 errs by at most gamma(n) sum|terms|, and so does any expression of rounding depth n by the same expression on
absolute values):
  z, eval out, g_x   gamma(n) S,  S = |A^T| [ (|G| |g| |G^T|) .* (|B^T| |d| |B|) ] |A| summed over the 32 input channels
                     (+ |bias|, + |skip|) under the tile alignment of the element (on the columns two segments share: the
                     larger of the two alignments' S).  n = N_CONV = 44:  32 (the K sum: sixteen 32x32x2 matrix steps, one
                     rounding per term) + 2 (input transform: rows, columns) + 4 (filter transform: two sums per stage, two
                     stages; the factors 1/2 are exact) + 1 (the product) + 2 (T = M A: two sums) + 2 (Y = A^T T: two sums) +
                     1 (bias / skip connection).  The inference block adds 4: scale, shift, slope, residual (N_EVAL = 48) on
                     |scale| S + |shift| + |x|.  The direct form's sum |x| |w| is NOT a bound here: the transforms create cross
                     terms.
  a_out              y = z sc + sh (2 roundings, or 1 fused), l = max(y, slope y) (1), a = l + skip (1):
                     u (1 + 4u) (|z sc| + |y| + |l| + |a|)
  g_z                gl = slope g_a (1), t = g - k1 (1), dm = z - mean (1), p = dm k2 (1, or fused), s = t - p (1), s k3 (1):
                     u (1 + 6u) (|k3| (|gl| + |t| + |dm k2| + |p| + |s|) + |g_z|); the branch is taken on the fp32
                     y = z sc + sh, so an element whose float64 |y| <= u (1 + 2u) (|z sc| + |y|) is UNDECIDED and accepted
                     against either branch (counted and capped by the tests)
  moments partial k  count exact; with n_l = 16 * the most units of a workgroup (values per lane), R = max |z - mean| over the
                     partial's pixels:  lane mean c + s1 / n: e_lane = gamma(n_l + 1) 2R + u |mean|;  after the 8-way Chan merge
                     (per merge: delta, ratio, product, sum)  e_mean = gamma(n_l + 30) 2R + 9u |mean|;
                     M2 = s2 - s1^2 / n per lane, merged:  e_M2 = 4 gamma(3 n_l + 56) n R^2 + 8 R e_lane n
  next sums partial k   per lane fp32 sums of n_l terms, then an exact double sum of 8:  sum g_y: gamma(n_l + 2) sum|g_y|;
                     sum g_y (z - mean): gamma(n_l + 3) sum|g_y| |z - mean|;  + (1 - slope) |g_x| (|z - mean|) of every element
                     undecided on y_next
  dW, db             a two-level sum: gamma(n1 + n2 + c) S_w,  n1 = 32 * the most units of a workgroup + 2 (tile terms of one
                     accumulator, the two halves of the matrix steps), n2 = the slabs (256), c = 9: 2 + 2 (both operand
                     transforms) + 1 (product) + 2 + 2 (the two output stages; the powers of two are exact), + 1 with accumulate;
                     S_w the F(3x3, 2x2) expression on absolute values, shared columns counted once.  db: gamma(32 * the most units of
                     a workgroup + 3 + n2 (+ 1)) sum|g_z|: a lane adds at most 32 row-pair sums per unit.

EXACT CASES.  B^T and A^T are signed sums, G carries factors 1/2: with small-integer operands the whole launch is exact in fp32
and must equal float64 bit for bit.  exact_headroom() returns the largest sum|terms| any accumulator of the restated algorithm
reaches, in units of the operands' quantum: an exact case needs it below 2^24.

The sum functions take a dtype and a `mut`: float64 is the restatement, float32 the emulation in the kernels' association
(transform, K sum, two-stage output transform); each MUTANT is one mistake an index path could make."""
import torch
import torch.nn.functional as F

U = 2.0 ** -24
SEG = 64
NAN = float("nan")
N_CONV = 44
N_EVAL = 48
N_WGRAD_C = 9
F64 = torch.float64

MUTANTS = {
    1: "dw_unowned",      # the neighbour of the shifted segment counts its unowned columns in dW / db
    2: "mom_unowned",     # ... in the BatchNorm moments
    3: "sums_unowned",    # ... in the next BatchNorm's sums
    4: "lone_clamped",    # the lone row of an odd comb is paired with the clamped row the kernel loads, not with zeros
    5: "midcomb_start",   # a workgroup range that begins mid-comb treats its row j0 - 1 like the start of a comb (zeros)
    6: "c0_no_bit",       # c0(t) without the inserted bit for d > 1
    7: "no_swap_d1",      # the d = 1 swap of column bits 0 and 1 left out of the gather
    8: "halo_wrapped",    # a halo column outside the image comes from the wrapped neighbouring row, not as zero
    9: "row_off_1",       # the row offset of a dilated tile is 1 instead of d
    10: "not_mirrored",   # the transposed filter is not mirrored
    11: "g_quarter",      # G's factor 1/4 applied to dW twice (("g_quarter", 2)) or not at all (("g_quarter", 0))
    12: "keep_mod",       # keep = W mod 64 where W is a multiple of 64
}


def gamma(n):
  return n * U / (1.0 - n * U)


def _kind(mut):
  return mut[0] if isinstance(mut, tuple) else mut


# ----------------------------------------------------------------------------- tiling
def nrows(H, d, r0):
  return -(-(H - r0) // d)


def comb_pairs(H, d, r0):
  return (nrows(H, d, r0) + 1) // 2


def pairs(H, d):
  return sum(comb_pairs(H, d, r) for r in range(d))


def nseg(W):
  return -(-W // SEG)


def units(B, H, W, d):
  return B * nseg(W) * pairs(H, d)


def wg_range(k, n, grid):
  return n * k // grid, n * (k + 1) // grid


def most_units(n, grid):
  return max(n * (k + 1) // grid - n * k // grid for k in range(grid))


def decode(u, H, W, d):
  """unit -> (image, segment, comb r0, pair), conv32_wino_kernel's order"""
  blk, pj = divmod(u, pairs(H, d))
  r0 = 0
  while pj >= comb_pairs(H, d, r0):
    pj -= comb_pairs(H, d, r0)
    r0 += 1
  b, seg = divmod(blk, nseg(W))
  return b, seg, r0, pj


def seg_start(seg, W, shifted=True):
  return min(SEG * seg, W - SEG) if shifted else SEG * seg


def seg_keep(seg, W, mut=None):
  ns = nseg(W)
  if seg == ns - 2 and (SEG * ns > W or _kind(mut) == "keep_mod"):
    return W - SEG * (ns - 1) if SEG * ns > W else W % SEG
  return SEG


def c0(t, d, mut=None):
  L = d.bit_length() - 1
  if _kind(mut) == "c0_no_bit":
    return t
  return ((t >> L) << (L + 1)) | (t & (d - 1))


def smallest_batch(H, W, d, floor=2048):
  return -(-floor // (nseg(W) * pairs(H, d)))


def owner_map(B, H, W, d, grid, shifted=True, mut=None, device="cpu"):
  """[B, H, W] int64: the workgroup that owns each pixel (-1: none), and `extra`: a second map of the pixels a mutant counts
  twice (None for the right restatement)."""
  ns, pp, n = nseg(W), pairs(H, d), units(B, H, W, d)
  y, x = torch.arange(H, device=device), torch.arange(W, device=device)
  offs = torch.tensor([sum(comb_pairs(H, d, r) for r in range(r0)) for r0 in range(d)], device=device)
  within = offs[y % d] + (y // d) // 2                                   # [H]
  seg = torch.where(x >= W - SEG, torch.full_like(x, ns - 1), x // SEG) if shifted else x // SEG
  b = torch.arange(B, device=device)

  def wg(segs):
    u = (b.view(B, 1, 1) * ns + segs.view(1, 1, W)) * pp + within.view(1, H, 1)
    return ((u + 1) * grid - 1) // n
  own = wg(seg)
  if _kind(mut) == "keep_mod" and W % SEG == 0 and ns >= 2:
    own[:, :, SEG * (ns - 2):SEG * (ns - 1)] = -1
  extra = None
  if _kind(mut) in ("dw_unowned", "mom_unowned", "sums_unowned") and SEG * ns > W and shifted:
    extra = torch.full_like(own, -1)
    extra[:, :, W - SEG:SEG * (ns - 1)] = wg(torch.full_like(x, ns - 2))[:, :, W - SEG:SEG * (ns - 1)]
  return own, extra


def owner_map_loop(B, H, W, d, grid, shifted=True):
  """the same map by walking the units of every workgroup, as the kernels do (for the CPU test)"""
  own = torch.full((B, H, W), -1, dtype=torch.int64)
  n = units(B, H, W, d)
  for k in range(grid):
    for u in range(*wg_range(k, n, grid)):
      b, seg, r0, pj = decode(u, H, W, d)
      x0 = seg_start(seg, W, shifted)
      keep = seg_keep(seg, W) if shifted else SEG
      for j in (2 * pj, 2 * pj + 1):
        if j < nrows(H, d, r0):
          own[b, r0 + j * d, x0:min(x0 + keep, W)] = k
  return own


def midcomb_starts(B, H, W, d, grid):
  """(image, segment, comb, pair) of every workgroup range that begins in the middle of a comb"""
  n = units(B, H, W, d)
  out = []
  for k in range(grid):
    u0, u1 = wg_range(k, n, grid)
    if u1 > u0:
      b, seg, r0, pj = decode(u0, H, W, d)
      if pj > 0:
        out.append((b, seg, r0, pj))
  return out


# ----------------------------------------------------------------------------- gathers
def _extend(x, E, dtype, wrapped):
  """[B, H, W + 2E, C]: the image with E columns either side — zeros, or (mutant) what lies there in the unpadded flat image"""
  B, H, W, C = x.shape
  if not wrapped:
    return F.pad(x.to(dtype), (0, 0, E, E))
  flat = F.pad(x.to(dtype).reshape(B, H * W, C), (0, 0, E, E))
  idx = torch.arange(H, device=x.device).view(H, 1) * W + torch.arange(W + 2 * E, device=x.device).view(1, -1)
  return flat[:, idx.reshape(-1)].reshape(B, H, W + 2 * E, C)


def _take_rows(xe, idx, clamp_bottom=False):
  """xe [B, H, Wx, C], idx [P, d] image rows -> [B, P, d, Wx, C]; rows outside the image are zero (mutant: the last row)"""
  B, H, Wx, C = xe.shape
  if clamp_bottom:
    idx = torch.where(idx >= H, torch.full_like(idx, H - 1), idx)
  bad = (idx < 0) | (idx >= H)
  xz = torch.cat([xe, torch.zeros(B, 1, Wx, C, dtype=xe.dtype, device=xe.device)], 1)
  return xz[:, torch.where(bad, torch.full_like(idx, H), idx).reshape(-1)].reshape(B, idx.shape[0], idx.shape[1], Wx, C)


def _take_cols(r, idx, W, E):
  """r [B, P, d, W + 2E, C], idx [Cb, d] image columns -> [B, P, d, Cb, d, C]; columns beyond the extension are zero"""
  B, P, dd, Wx, C = r.shape
  bad = (idx < -E) | (idx >= W + E)
  rz = torch.cat([r, torch.zeros(B, P, dd, 1, C, dtype=r.dtype, device=r.device)], 3)
  return rz[:, :, :, torch.where(bad, torch.full_like(idx, Wx - E), idx).reshape(-1) + E].reshape(B, P, dd, idx.shape[0], idx.shape[1], C)


def _swap01(v):
  return (v & ~3) | ((v & 1) << 1) | ((v >> 1) & 1)


def _tile_index(H, d, col0, ncols, mut, device):
  """row index [P, d] of tile row m = 1 (the pair's first row) and column index [Cb, d] of tile column n = 1"""
  P, Cb = -(-H // (2 * d)), ncols // (2 * d)
  rows = torch.arange(P, device=device).view(P, 1) * 2 * d + torch.arange(d, device=device).view(1, d)
  t = torch.arange(Cb, device=device).view(Cb, 1) * d + torch.arange(d, device=device).view(1, d)
  L = d.bit_length() - 1
  rel = t if (_kind(mut) == "c0_no_bit" and d > 1) else ((t >> L) << (L + 1)) | (t & (d - 1))
  return rows, rel + col0


def _sub(absolute):
  return (lambda a, b: a + b) if absolute else (lambda a, b: a - b)


def _in_transform(xe, H, W, d, E, col0, ncols, absolute, mut, wgrad=False, zero_row0=()):
  """V[r][c] = (B^T X B)[r][c] of every 4x4 input tile of the column range [col0, col0 + ncols): rows first, then columns, one
  rounding each — [B, P, d, Cb, d, C] per entry"""
  s = _sub(absolute)
  rows, cols = _tile_index(H, d, col0, ncols, mut, xe.device)
  step = 1 if _kind(mut) == "row_off_1" else d
  X = [_take_rows(xe, rows + (m - 1) * step, clamp_bottom=(_kind(mut) == "lone_clamped" and m >= 2)) for m in range(4)]
  for (b, x0, r0, pj) in zero_row0:
    X[0][b, pj, r0, max(E + x0 - d, 0):E + x0 + SEG + d] = 0
  R = [s(X[0], X[2]), X[1] + X[2], s(X[2], X[1]), s(X[3], X[1]) if wgrad else s(X[1], X[3])]
  del X
  V = []
  for r in range(4):
    C = []
    for n in range(4):
      idx = cols + (n - 1) * d
      if _kind(mut) == "no_swap_d1" and d == 1:
        idx = _swap01(idx - col0 + 8) - 8 + col0
      C.append(_take_cols(R[r], idx, W, E))
    V.append([s(C[0], C[2]), C[1] + C[2], s(C[2], C[1]), s(C[3], C[1]) if wgrad else s(C[1], C[3])])
  return V


def _g_row(r, x0, x1, x2, s):
  return x0 if r == 0 else (x2 if r == 3 else (0.5 * ((x0 + x2) + x1) if r == 1 else 0.5 * s(x0 + x2, x1)))


def filter_transform(w, transposed=False, dtype=F64, absolute=False, mut=None):
  """as_conv32_wino_pack_weights: U[r][c] = (G g G^T)[r][c] as [ci][co] matrices; transposed: the data gradient's filter
  (channels swapped, taps mirrored); columns first, then rows, as wino_pack_one"""
  s = _sub(absolute)
  w = w.to(dtype)
  if transposed:
    w = w.transpose(0, 1)
    if _kind(mut) != "not_mirrored":
      w = w.flip(2, 3)
  col = [[_g_row(c, w[:, :, a, 0], w[:, :, a, 1], w[:, :, a, 2], s) for c in range(4)] for a in range(3)]
  return [[_g_row(r, col[0][c], col[1][c], col[2][c], s).t().contiguous() for c in range(4)] for r in range(4)]


def _wino_range(xe, Uw, H, W, d, E, col0, ncols, absolute, mut, zero_row0=()):
  s = _sub(absolute)
  V = _in_transform(xe, H, W, d, E, col0, ncols, absolute, mut, zero_row0=zero_row0)
  T = []
  for r in range(4):
    M = [torch.matmul(V[r][c], Uw[r][c]) for c in range(4)]
    V[r] = None
    T.append([(M[0] + M[1]) + M[2], s(s(M[1], M[2]), M[3])])
  Y = [[(T[0][j] + T[1][j]) + T[2][j] for j in range(2)], [s(s(T[1][j], T[2][j]), T[3][j]) for j in range(2)]]
  out = torch.stack([torch.stack(Y[0], 4), torch.stack(Y[1], 4)], 2)         # [B, P, oi, d, Cb, oj, d, Co]
  B = out.shape[0]
  return out.reshape(B, -1, ncols, out.shape[-1])[:, :H]


def conv_wino(x, w, d, dtype=F64, transposed=False, absolute=False, mut=None, grid=None):
  """The convolution (transposed: the data gradient) of x by F(2x2, 3x3) in the kernels' tiling and association.  absolute:
  the same expression on absolute values — pass |x|, |w| — with the larger of the two alignments on shared columns.  mut: one
  of MUTANTS 4 - 10, 12 (5 needs `grid`).  A pixel the mutant never writes is NaN."""
  B, H, W, _ = x.shape
  ns, E = nseg(W), 2 * d + 8
  xe = _extend(x, E, dtype, _kind(mut) == "halo_wrapped")
  Uw = filter_transform(w, transposed, dtype, absolute, mut)
  Uw = [[u.to(x.device) for u in row] for row in Uw]
  starts = midcomb_starts(B, H, W, d, grid) if _kind(mut) == "midcomb_start" else []
  z0 = lambda segs: [(b, seg_start(sg, W), r0, pj) for (b, sg, r0, pj) in starts if sg in segs]
  if SEG * ns > W:
    main = _wino_range(xe, Uw, H, W, d, E, 0, SEG * (ns - 1), absolute, mut, z0(range(ns - 1)))
    last = _wino_range(xe, Uw, H, W, d, E, W - SEG, SEG, absolute, mut, z0([ns - 1]))
    out = torch.cat([main[:, :, :W - SEG], last], 2)
    if absolute:
      out[:, :, W - SEG:SEG * (ns - 1)] = torch.maximum(main[:, :, W - SEG:], last[:, :, :SEG * ns - W])
  else:
    out = _wino_range(xe, Uw, H, W, d, E, 0, W, absolute, mut, z0(range(ns)))
    if _kind(mut) == "keep_mod" and ns >= 2:
      out[:, :, SEG * (ns - 2):SEG * (ns - 1)] = NAN
  return out


def _eff(w, transposed, dtype):
  w = w.to(dtype)
  return w.transpose(0, 1).flip(2, 3) if transposed else w


def conv_direct(x, w, d, dtype=F64, transposed=False):
  """the same convolution in its direct form: nine taps, zero padding"""
  B, H, W, _ = x.shape
  we = _eff(w, transposed, dtype).to(x.device)
  xp = F.pad(x.to(dtype), (0, 0, d, d, d, d))
  out = torch.zeros(B, H, W, we.shape[0], dtype=dtype, device=x.device)
  for a in range(3):
    for b in range(3):
      if bool(we[:, :, a, b].any()):
        out += torch.matmul(xp[:, a * d:a * d + H, b * d:b * d + W], we[:, :, a, b].t())
  return out


# ----------------------------------------------------------------------------- weight gradient F(3x3, 2x2)
def _wgrad_M(xe, gz, H, W, d, E, col0, ncols, absolute, mut):
  """M[r][c][ci][co] = sum over the tiles of the column range of (B^T x B)[r][c][ci] (G g G^T without its halves)[r][c][co]"""
  s = _sub(absolute)
  V = _in_transform(xe, H, W, d, E, col0, ncols, absolute, mut, wgrad=True)
  rows, cols = _tile_index(H, d, col0, ncols, mut, gz.device)
  g = [_take_rows(gz, rows + i * d) for i in range(2)]
  Gr = [g[0], g[0] + g[1], s(g[0], g[1]), g[1]]
  M = []
  for r in range(4):
    Gc = [_take_cols(Gr[r], cols + jc * d, W, 0) for jc in range(2)]
    Gt = [Gc[0], Gc[0] + Gc[1], s(Gc[0], Gc[1]), Gc[1]]
    C = gz.shape[-1]
    M.append([torch.matmul(V[r][c].reshape(-1, C).t(), Gt[c].reshape(-1, C)) for c in range(4)])
  return M


def wgrad_wino(x, gz, d, dtype=F64, shifted=True, absolute=False, mut=None):
  """dW [co][ci][3][3], db [co] and the largest |accumulator| bound max sum|V||G| — the weight gradient by F(3x3, 2x2): the sum
  over tiles is the K dimension; the halves of G are applied once, at the end, then (M A) and A^T.  shifted: the fused
  backward's segments (the neighbour of the shifted segment reads its unowned g_z columns as zero); else the stand-alone
  kernel's (no shift, zero beyond the image edge)."""
  s = _sub(absolute)
  B, H, W, C = x.shape
  ns, E = nseg(W), 2 * d + 8
  xe = _extend(x, E, dtype, False)
  g = gz.to(dtype)
  if _kind(mut) == "keep_mod" and shifted and W % SEG == 0 and ns >= 2:
    g = g.clone()
    g[:, :, SEG * (ns - 2):SEG * (ns - 1)] = 0
  if shifted and SEG * ns > W:
    gm = g.clone()
    if _kind(mut) != "dw_unowned":
      gm[:, :, W - SEG:] = 0
    else:
      gm[:, :, SEG * (ns - 1):] = 0
    Ms = [_wgrad_M(xe, gm, H, W, d, E, 0, SEG * (ns - 1), absolute, mut), _wgrad_M(xe, g, H, W, d, E, W - SEG, SEG, absolute, mut)]
    db = gm.sum((0, 1, 2)) + g[:, :, W - SEG:].sum((0, 1, 2))
  else:
    Ms = [_wgrad_M(xe, g, H, W, d, E, 0, SEG * ns, absolute, mut)]
    db = g.sum((0, 1, 2))
  M = [[sum(m[r][c] for m in Ms) for c in range(4)] for r in range(4)]
  peak = max(float(M[r][c].abs().max()) for r in range(4) for c in range(4))
  q = 1.0
  if _kind(mut) == "g_quarter":
    q = 0.25 if mut[1] == 2 else 4.0
  ex = []
  for r in range(4):
    sr = 0.5 if r in (1, 2) else 1.0
    m0, m1, m2, m3 = (q * sr) * M[r][0], (q * 0.5 * sr) * M[r][1], (q * 0.5 * sr) * M[r][2], (q * sr) * M[r][3]
    ex.append([(m0 + m1) + m2, s(m1, m2), (m1 + m2) + m3])
  dW = torch.zeros(C, C, 3, 3, dtype=dtype, device=x.device)
  for b in range(3):
    col = [(ex[0][b] + ex[1][b]) + ex[2][b], s(ex[1][b], ex[2][b]), (ex[1][b] + ex[2][b]) + ex[3][b]]
    for a in range(3):
      dW[:, :, a, b] = col[a].t()
  return dW, db, peak


def wgrad_direct(x, gz, d, dtype=F64):
  B, H, W, C = x.shape
  xp, g = F.pad(x.to(dtype), (0, 0, d, d, d, d)), gz.to(dtype).reshape(-1, C)
  dW = torch.zeros(C, C, 3, 3, dtype=dtype, device=x.device)
  for a in range(3):
    for b in range(3):
      dW[:, :, a, b] = torch.matmul(g.t(), xp[:, a * d:a * d + H, b * d:b * d + W].reshape(-1, C))
  return dW, g.sum(0)


# ----------------------------------------------------------------------------- element-wise chains
def _c(v, dtype=F64):
  return v.to(dtype).view(1, 1, 1, -1)


def f32(v):
  """the float the kernels receive for a host-side number such as the slope, widened"""
  return float(torch.tensor(v, dtype=torch.float32))


def act_chain(z_prev, skip, sc, sh, slope, dtype=F64):
  """a_out = lrelu(z_prev sc + sh) (+ skip) and its bound"""
  slope = f32(slope)
  z = z_prev.to(dtype)
  y = z * _c(sc, dtype).to(z.device) + _c(sh, dtype).to(z.device)
  l = torch.maximum(y, y * slope)
  a = l + skip.to(dtype) if skip is not None else l
  e = U * (1 + 4 * U) * ((z * _c(sc, dtype).to(z.device)).abs() + y.abs() + l.abs() + (a.abs() if skip is not None else 0.0))
  return a, e


def gz_chain(g_a, z, sc, sh, mean, coef, slope, dtype=F64):
  """g_z = (g_y - k1 - (z - mean) k2) k3, g_y = g_a where y = z sc + sh > 0 else slope g_a: both branches with their bounds,
  the branch float64 takes and the UNDECIDED mask.  In float32 the branch is the float32 y's."""
  dev, slope = z.device, f32(slope)
  ga, zz = g_a.to(dtype), z.to(dtype)
  k1, k2, k3 = (_c(coef[32 * i:32 * i + 32], dtype).to(dev) for i in range(3))
  zs = zz * _c(sc, dtype).to(dev)
  y = zs + _c(sh, dtype).to(dev)
  e_y = U * (1 + 2 * U) * (zs.abs() + y.abs())
  dm = zz - _c(mean, dtype).to(dev)
  p = dm * k2
  out = {}
  for name, gy, extra in (("pos", ga, 0.0), ("neg", ga * slope, (ga * slope).abs())):
    t = gy - k1
    s_ = t - p
    gz = s_ * k3
    out[name] = gz
    out["e_" + name] = U * (1 + 6 * U) * (k3.abs() * (extra + t.abs() + 2 * p.abs() + s_.abs()) + gz.abs())
  out["positive"] = y > 0
  out["undecided"] = y.abs() <= e_y
  out["g_z"] = torch.where(out["positive"], out["pos"], out["neg"])
  return out


def judge_gz(got, ref):
  """worst err / bound of a g_z against gz_chain's result: decided elements against their branch, undecided ones against
  the nearer branch; returns (ratio, undecided count)"""
  g = got.double()
  r_pos = (g - ref["pos"]).abs() / ref["e_pos"].clamp(min=1e-300)
  r_neg = (g - ref["neg"]).abs() / ref["e_neg"].clamp(min=1e-300)
  r = torch.where(ref["undecided"], torch.minimum(r_pos, r_neg), torch.where(ref["positive"], r_pos, r_neg))
  return float(r.nan_to_num(float("inf")).max()), int(ref["undecided"].sum())


# ----------------------------------------------------------------------------- restatement + bound of each launch
def forward_z(a32, w, bias, d):
  """z = conv(a_out) + bias from the launch's own fp32 a_out, and gamma(N_CONV) S"""
  dev = a32.device
  z = conv_direct(a32, w, d)
  S = conv_wino(a32.abs(), w.abs(), d, absolute=True)
  if bias is not None:
    z, S = z + _c(bias).to(dev), S + _c(bias).abs().to(dev)
  return dict(z=z, e_z=gamma(N_CONV) * S, S=S)


def eval_out(x, w, bias, scale, shift, slope, residual, d):
  dev, slope = x.device, f32(slope)
  f = forward_z(x, w, bias, d)
  y = f["z"] * _c(scale).to(dev) + _c(shift).to(dev)
  out = torch.maximum(y, y * slope)
  S = f["S"] * _c(scale).abs().to(dev) + _c(shift).abs().to(dev)
  if residual:
    out, S = out + x.double(), S + x.double().abs()
  return dict(out=out, e_out=gamma(N_EVAL) * S)


def data_gradient(gz32, g_a, w, d):
  """g_x = dgrad(g_z) + g_a from the launch's own fp32 g_z"""
  gx = conv_direct(gz32, w, d, transposed=True) + g_a.double()
  S = conv_wino(gz32.abs(), w.abs(), d, transposed=True, absolute=True) + g_a.double().abs()
  return dict(g_x=gx, e_g_x=gamma(N_CONV) * S)


def _scatter(v, own, grid):
  C = v.shape[-1]
  o = own.reshape(-1)
  ok = o >= 0
  return torch.zeros(grid, C, dtype=F64, device=v.device).index_add_(0, o[ok], v.reshape(-1, C)[ok])


def _scatter_max(v, own, grid):
  C = v.shape[-1]
  o = own.reshape(-1)
  ok = o >= 0
  return torch.zeros(grid, C, dtype=F64, device=v.device).scatter_reduce_(
      0, o[ok].view(-1, 1).expand(-1, C), v.reshape(-1, C)[ok], "amax", include_self=True)


def _both(fn, own, extra):
  r = fn(own)
  return r + fn(extra) if extra is not None else r


def moments(z32, d, grid, mut=None):
  """(count [grid], mean, M2 [grid][32]) of workgroup k's owned pixels of the launch's own fp32 z, with bounds"""
  B, H, W, C = z32.shape
  z = z32.double()
  own, extra = owner_map(B, H, W, d, grid, True, mut if _kind(mut) in ("mom_unowned", "keep_mod") else None, z.device)
  one = torch.ones(B, H, W, 1, dtype=F64, device=z.device)
  cnt = _both(lambda o: _scatter(one, o, grid), own, extra)[:, 0]
  n = cnt.clamp(min=1).view(-1, 1)
  mean = _both(lambda o: _scatter(z, o, grid), own, extra) / n
  dev = lambda o: (z - mean[o.clamp(min=0)]) * (o >= 0).unsqueeze(-1)
  m2 = _both(lambda o: _scatter(dev(o) ** 2, o, grid), own, extra)
  R = _scatter_max(dev(own).abs(), own, grid)
  nl = 16 * most_units(units(B, H, W, d), grid)
  e_lane = gamma(nl + 1) * 2 * R + U * mean.abs()
  e_mean = gamma(nl + 30) * 2 * R + 9 * U * mean.abs()
  e_m2 = 4 * gamma(3 * nl + 56) * n * R * R + 8 * R * e_lane * n
  return dict(cnt=cnt, mean=mean, m2=m2, e_mean=e_mean, e_m2=e_m2)


def next_sums(gx32, z_next, n_scale, n_shift, n_mean, slope, d, grid, mut=None):
  """[grid][64]: sum g_y and sum g_y (z_next - mean) over workgroup k's owned pixels of the launch's own fp32 g_x, with bounds
  and the count of elements undecided on y_next"""
  B, H, W, C = gx32.shape
  dev, slope = gx32.device, f32(slope)
  gx, zn = gx32.double(), z_next.double()
  zs = zn * _c(n_scale).to(dev)
  y = zs + _c(n_shift).to(dev)
  und = y.abs() <= U * (1 + 2 * U) * (zs.abs() + y.abs())
  gy = torch.where(y > 0, gx, gx * slope)
  dm = zn - _c(n_mean).to(dev)
  slack = torch.where(und, gx.abs() * (1 - slope), torch.zeros_like(gx))
  own, extra = owner_map(B, H, W, d, grid, True, mut if _kind(mut) in ("sums_unowned", "keep_mod") else None, dev)
  sc = lambda v: _both(lambda o: _scatter(v, o, grid), own, extra)
  nl = 16 * most_units(units(B, H, W, d), grid)
  sums = torch.cat([sc(gy), sc(gy * dm)], 1)
  e = torch.cat([gamma(nl + 2) * sc(gy.abs()) + sc(slack), gamma(nl + 3) * sc((gy * dm).abs()) + sc(slack * dm.abs())], 1)
  return dict(sums=sums, e_sums=e, undecided=int(und.sum()))


def weight_gradient(x, gz32, d, grid, shifted, dW0=None, db0=None, slabs=256):
  """dW, db from x and the two-launch fp32 g_z, gamma(n1 + n2 + c) S_w"""
  B, H, W, C = x.shape
  dW, db = wgrad_direct(x, gz32, d)
  SW, Sb, _ = wgrad_wino(x.abs(), gz32.abs(), d, shifted=shifted, absolute=True)
  mu = most_units(units(B, H, W, d), grid)
  c = N_WGRAD_C
  if dW0 is not None:
    dW, db, SW, Sb, c = dW + dW0.double().to(x.device), db + db0.double().to(x.device), SW + dW0.double().abs().to(x.device), \
        Sb + db0.double().abs().to(x.device), c + 1
  # (db: a lane adds at most 32 row-pair sums per unit — 16 matrix steps, two columns — each one rounding, + the merge of the
  #  halves, + the slabs)
  return dict(dW=dW, db=db, e_dW=gamma(32 * mu + 2 + slabs + c) * SW, e_db=gamma(32 * mu + 3 + slabs + (1 if dW0 is not None else 0)) * Sb)


def exact_headroom(x, w, d, qx, qw, transposed=False):
  """largest sum|terms| of any accumulator of conv_wino on this integer case, in units of the products' quantum qx qw / 4 (x a
  multiple of qx, w of qw: U = G g G^T a multiple of qw / 4): exact in fp32 when below 2^24.  The absolute-value form bounds
  every intermediate: the output transforms only add."""
  S = conv_wino(x.abs(), w.abs(), d, transposed=transposed, absolute=True)
  return float(S.max()) / (qx * qw / 4)


def exact_headroom_wgrad(x, gz, d, qx, qg, shifted):
  """the same for the weight gradient: the accumulators hold sums of (B^T x B)(G' g G'^T) — multiples of qx qg — and the slab
  values are those times 1/4"""
  SW, Sb, peak = wgrad_wino(x.abs(), gz.abs(), d, shifted=shifted, absolute=True)
  return max(peak / (qx * qg), float(SW.max()) / (qx * qg / 4), float(Sb.max()) / qg)


def ratio(got, ref, bound):
  """worst |got - ref| / bound; a NaN in got (never written, or a guard value consumed) counts as infinite"""
  got, ref = got.double().reshape(ref.shape), ref.double()
  q = ((got - ref).abs() / bound.double().reshape(ref.shape).clamp(min=1e-300))
  q = torch.where((got == ref), torch.zeros_like(q), q)
  return float(q.nan_to_num(float("inf")).max())


# ----------------------------------------------------------------------------- the cases
DILATIONS = (1, 2, 4, 8)


def geometries(d, floor=2048, scale=1):
  """(B, H, W) of the issue's table for dilation d: the smallest batch with units >= floor.  scale > 1 (the CPU file): the same
  H and W with a floor `scale` times lower."""
  out = []
  for H, W in ((2 * d, 64), (2 * d + 1, 65), (2 * d, 129), (37, 127), (51, 192), (23 + d, 191)):
    out.append((smallest_batch(H, W, d, floor // scale), H, W))
  return out


def geom_id(g):
  return "%dx%dx%d" % tuple(g)


def _gen(seed, device):
  return torch.Generator(device=device).manual_seed(seed)


def _seed(geom, d, k):
  B, H, W = geom
  return 100003 * k + 7 * B + 131 * H + W + 17 * d


def _sentinels(t, val=1e4):
  t[:, 0] = val; t[:, -1] = -val; t[:, :, 0] = -val; t[:, :, -1] = val
  return t


def _state(seed, device):
  g = _gen(seed, "cpu")
  mean = torch.randn(32, generator=g) * 0.1
  invstd = torch.randn(32, generator=g).abs() + 0.5
  scale = invstd * (torch.randn(32, generator=g).abs() + 0.5)
  shift = torch.randn(32, generator=g) * 0.1 - mean * scale
  return dict(mean=mean.to(device), scale=scale.to(device), shift=shift.to(device))


def case(geom, d, fam, device="cpu"):
  """The operands of one geometry and family, fp32 on `device`:
    random   N(0, 1) tensors, weights N(0, 1) * 0.06, +-1e4 sentinels on the first and last rows and columns of every input
    offset   the same without sentinels, + 1e3 on z_prev and on the bias (the moments' pivot)"""
  B, H, W = geom
  T = lambda k: torch.randn(B, H, W, 32, generator=_gen(_seed(geom, d, k), device), device=device)
  c = {n: T(k) for k, n in enumerate(("z_prev", "a_pp", "x", "g_a", "z", "z_next"))}
  g = _gen(_seed(geom, d, 9), "cpu")
  c["w"] = torch.randn(32, 32, 3, 3, generator=g) * 0.06
  c["b"] = torch.randn(32, generator=g) * 0.1
  c["coef"] = torch.randn(96, generator=g) * 0.05
  c["coef"][64:] = c["coef"][64:].abs() + 0.7
  c["st_in"], c["st"], c["st_next"] = _state(_seed(geom, d, 10), device), _state(_seed(geom, d, 11), device), _state(_seed(geom, d, 12), device)
  if fam == "random":
    for n in ("z_prev", "a_pp", "x", "g_a", "z", "z_next"):
      _sentinels(c[n])
  elif fam == "offset":
    c["z_prev"] += 1e3
    c["b"] = c["b"] + 1e3
  else:
    raise ValueError(fam)
  for n in ("w", "b", "coef"):
    c[n] = c[n].to(device)
  c["slope"] = 0.2
  return c


EXACT_WEIGHTS = [("tap", t) for t in range(9)] + [("dense", 0)]


def exact_case(geom, d, wfam, device="cpu"):
  """The integer family: operands in {-1, 0, 1} thinned to a third, slope 0.5, scales that are powers of two, k1 = k2 = 0,
  k3 = 2; wfam ("tap", t): w[:, :, t / 3, t % 3] a thinned +-1 matrix, every other tap zero; ("dense", 0): all nine taps."""
  B, H, W = geom
  def T(k):
    g = _gen(_seed(geom, d, 20 + k), device)
    v = torch.randint(-1, 2, (B, H, W, 32), generator=g, device=device).float()
    return v * (torch.rand(B, H, W, 32, generator=g, device=device) < 0.34).float()
  c = {n: T(k) for k, n in enumerate(("z_prev", "a_pp", "x", "g_a", "z", "z_next"))}
  g = _gen(_seed(geom, d, 29) + 31 * wfam[1], "cpu")
  w = torch.randint(-1, 2, (32, 32, 3, 3), generator=g).float() * (torch.rand(32, 32, 3, 3, generator=g) < 0.5).float()
  if wfam[0] == "tap":
    keep = torch.zeros(3, 3)
    keep[wfam[1] // 3, wfam[1] % 3] = 1
    w = w * keep
  c["w"] = w.to(device)
  c["b"] = torch.randint(-2, 3, (32,), generator=g).float().to(device)
  coef = torch.zeros(96)
  coef[64:] = 2.0
  c["coef"] = coef.to(device)
  pw2 = torch.pow(2.0, (torch.arange(32) % 3 - 1).float())
  st = lambda sh: dict(mean=torch.zeros(32, device=device), scale=pw2.to(device), shift=torch.full((32,), sh, device=device))
  c["st_in"], c["st"], c["st_next"] = st(0.5), st(-0.5), st(0.5)
  c["slope"] = 0.5
  return c
