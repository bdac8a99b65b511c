// Semi-global matching beside the network: census transform, Hamming cost, path aggregation, winner selection for both views out
// of one volume.  The four entry points are CONTRACTS (include/adaptive_stereo_hip.h, restated in numpy by tests/sgm_ref.py): all
// integer arithmetic up to the sub-pixel division, so every result is exact whatever order the work runs in.
//
//   sgm_census_kernel    a workgroup covers SGM_CEN_H = 8 rows x SGM_CEN_W = 32 columns: the quantised grey values of the tile and
//                        its 3-row / 4-column halo (clamped to the image) go to LDS once, then one lane per pixel compares its 62
//                        neighbours out of LDS and stores one 64-bit word.
//
// The aggregation and the selection share one lane layout.  A pixel's D disparities lie SGM_PER_LANE = 4 to a lane, d = 4 * j + k,
// over a GROUP of G lanes, G the smallest power of two with 4 * G >= D (G = 64 at D = 192 .. 256: one pixel a wave; G = 1 at D <= 4:
// 64 pixels a wave).  Groups are aligned in the wave, so __shfl_xor over offsets below G stays inside one, and a lane's d - 1 / d + 1
// neighbours that are not its own are its neighbour lanes' (__shfl_up / __shfl_down by 1).  Nothing goes through LDS.  A lane's four
// values of S are 8 contiguous bytes; when D % 4 == 0 they are one 8-byte access (VEC), otherwise four 2-byte ones.  Entries with
// d >= D carry SGM_FAR, which loses every minimum and is never stored.
//
//   sgm_rows_kernel      the two horizontal paths: a group walks one row from left to right storing S = L, then from right to left
//                        adding its L: the launch that initialises S.  B * H lines.
//   sgm_cols_kernel      one vertical or diagonal path (dy, dx): a group walks a column line, x advancing by dx per row and wrapping
//                        modulo W with the recurrence reset at the wrap, and adds its L to S.  B * W lines of H pixels; the groups
//                        of a wave hold neighbouring lines, whose pixels are neighbours in memory at every step.
//                        Both walk their line in chunks of 8 pixels: what a chunk reads (census words, and S where it adds; none of
//                        it depends on the recurrence) is requested before its first step, so the dependent chain of the steps
//                        waits for memory once a chunk.  Measured at 4 x 375 x 1242, D = 192: one pixel at a time 7.7 ms for eight
//                        paths, in chunks 5.4 ms (profiles/sgm_timing.txt).
//   sgm_select_kernel    a group per pixel: the left column S(y,x,.) and the right one S(y,x+d,d), arg-min by a min over
//                        (value << 9 | d) across the group, the uniqueness test as an OR across it, the two neighbours of the winner
//                        fetched from the lanes that hold them.  The counts go the way of code_maps.h (as_counts_*).
#include "code_maps.h"

#pragma clang fp contract(off)

#define SGM_CEN_W 32
#define SGM_CEN_H 8
#define SGM_HALO_X 4
#define SGM_HALO_Y 3
#define SGM_CEN_LW (SGM_CEN_W + 2 * SGM_HALO_X)
#define SGM_CEN_LH (SGM_CEN_H + 2 * SGM_HALO_Y)
#define SGM_BLOCK 256
#define SGM_PER_LANE 4
#define SGM_MAX_D 256
#define SGM_ROW_CHUNK 8             // pixels of a horizontal path whose loads are in flight together
#define SGM_COL_CHUNK 8             // ... of a vertical or diagonal one (no right word is shared between its pixels)
#define SGM_FAR 0x3FFF              // an absent disparity's path cost: above every real one (<= 64 + 255), small enough to add to
#define SGM_OUT_OF_VIEW 64          // the matching cost where x - d < 0
#define SGM_CODES 8                 // 0 keep, 1-6 as as_disp_speckle's table, 7 not unique
#define SGM_GROUPS 2048             // workgroups of a launch (8 a CU: every one resident at once)

typedef unsigned short sgm_u16x4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------------------------------------ census
struct SgmCensusArgs {
  const float* img;
  uint64_t* census;
  int C, H, W, xtiles;
  long tiles;
};

__global__ __launch_bounds__(SGM_BLOCK) void sgm_census_kernel(SgmCensusArgs a) {
  __shared__ uint8_t q[SGM_CEN_LH][SGM_CEN_LW];
  const int H = a.H, W = a.W;
  const long plane = (long)H * W;
  const float* I = a.img + (long)blockIdx.y * a.C * plane;
  uint64_t* out = a.census + (long)blockIdx.y * plane;
  const int lx = threadIdx.x & (SGM_CEN_W - 1), ly = threadIdx.x / SGM_CEN_W;
  for (long tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
    const long ty = tile / a.xtiles;
    const long y0 = ty * SGM_CEN_H, x0 = (tile - ty * a.xtiles) * SGM_CEN_W;
    __syncthreads();                                                   // the tile before this one has been read
    for (int i = threadIdx.x; i < SGM_CEN_LH * SGM_CEN_LW; i += SGM_BLOCK) {
      const int iy = i / SGM_CEN_LW, ix = i - iy * SGM_CEN_LW;
      const long yy = min(max(y0 + iy - SGM_HALO_Y, 0L), (long)H - 1), xx = min(max(x0 + ix - SGM_HALO_X, 0L), (long)W - 1);
      const long at = yy * W + xx;
      float g;
      if (a.C == 3) {
        const float rg = 0.299f * I[at] + 0.587f * I[plane + at];
        g = rg + 0.114f * I[2 * plane + at];
      } else {
        g = I[at];
      }
      const float v = g * 255.0f + 0.5f;
      q[iy][ix] = (uint8_t)(int)floorf(fminf(fmaxf(v, 0.0f), 255.0f));   // fmaxf(NaN, 0) = 0
    }
    __syncthreads();
    const long y = y0 + ly, x = x0 + lx;
    if (y >= H || x >= W) continue;                                    // no barrier depends on this lane's path: both are above
    const int c = q[ly + SGM_HALO_Y][lx + SGM_HALO_X];
    uint64_t w = 0;
#pragma unroll
    for (int dy = 0; dy < 2 * SGM_HALO_Y + 1; ++dy)
#pragma unroll
      for (int dx = 0; dx < 2 * SGM_HALO_X + 1; ++dx) {
        const int k = dy * (2 * SGM_HALO_X + 1) + dx;
        if (k == 31) continue;                                         // the centre
        // the tile's clamped halo is the clamp of the pixel's own window: rows and columns beyond the image repeat its border
        w |= (uint64_t)(q[ly + dy][lx + dx] < c) << k;
      }
    out[y * W + x] = w;
  }
}

static int sgm_check_volume(const char* who, int B, int H, int W, int D) {
  if (int rc = as_check_images(who, B, H, W, false)) return rc;              // H * W * D below bounds H * W
  AS_CHECK_ARG(D >= 1 && D <= SGM_MAX_D, "%s: D %d outside 1 .. %d", who, D, SGM_MAX_D);
  AS_CHECK_ARG((int64_t)H * W * D <= 0x7FFFFFFF, "%s: H * W * D = %lld overflows an int32 index into an image's volume", who,
               (long long)H * W * D);
  return AS_OK;
}

extern "C" int as_sgm_census(const float* img, int B, int C, int H, int W, uint64_t* census, void* stream) {
  AS_CHECK_ARG(img && census, "as_sgm_census: null pointer");
  if (int rc = as_check_images("as_sgm_census", B, H, W, true)) return rc;
  AS_CHECK_ARG(C == 1 || C == 3, "as_sgm_census: C %d outside {1, 3}", C);
  AS_CHECK_ARG(((uintptr_t)census & 7) == 0 && ((uintptr_t)img & 3) == 0,
               "as_sgm_census: census must be 8-byte aligned and img 4-byte aligned");
  const int64_t n = (int64_t)B * H * W;
  const AsRange r[] = {{img, n * C * 4}, {census, n * 8}};
  AS_CHECK_ARG(as_disjoint(r, 1, 2), "as_sgm_census: the output may not alias the input (overlapping ranges)");
  SgmCensusArgs a;
  a.img = img; a.census = census; a.C = C; a.H = H; a.W = W;
  a.xtiles = as_div_up(W, SGM_CEN_W);
  a.tiles = (long)as_div_up(H, SGM_CEN_H) * a.xtiles;
  hipLaunchKernelGGL(sgm_census_kernel, as_strided_grid(a.tiles, 4 * SGM_GROUPS, B), dim3(SGM_BLOCK), 0, (hipStream_t)stream, a);
  AS_CHECK_LAUNCH("as_sgm_census");
  return AS_OK;
}

// ------------------------------------------------------------------------------------------------ aggregation
extern "C" int64_t as_sgm_workspace(int B, int H, int W, int D) {
  if (B <= 0 || H <= 0 || W <= 0 || B > 65535 || D < 1 || D > SGM_MAX_D || (int64_t)H * W * D > 0x7FFFFFFF) return 0;
  return (int64_t)B * H * W * D * 2;
}

struct SgmAggArgs {
  const uint64_t* cl;
  const uint64_t* cr;
  uint16_t* S;
  long lines;                       // B * H (rows) or B * W (columns)
  int H, W, D, P1, P2, dy, dx;
};

// the matching cost of the lane's four disparities at column x from the census words in registers: l the left word, r[k] the
// right word at x - d0 - k (whatever where that lies outside the row)
static __device__ inline void sgm_cost(int (&C)[SGM_PER_LANE], uint64_t l, uint64_t r0, uint64_t r1, uint64_t r2, uint64_t r3, int x,
                                       int d0, int D) {
  const uint64_t r[SGM_PER_LANE] = {r0, r1, r2, r3};
#pragma unroll
  for (int k = 0; k < SGM_PER_LANE; ++k) {
    const int d = d0 + k;
    C[k] = d >= D ? SGM_FAR : x - d >= 0 ? __popcll(l ^ r[k]) : SGM_OUT_OF_VIEW;
  }
}

// L <- C + min(L[d], L[d-1] + P1, L[d+1] + P1, m + P2) - m over the group, or L <- C at the start of a path
template <int G>
static __device__ inline void sgm_step(int (&L)[SGM_PER_LANE], const int (&C)[SGM_PER_LANE], bool reset, int d0, int D, int P1,
                                       int P2) {
  int m = min(min(L[0], L[1]), min(L[2], L[3]));
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) m = min(m, __shfl_xor(m, o, 64));
  int below = __shfl_up(L[SGM_PER_LANE - 1], 1, 64), above = __shfl_down(L[0], 1, 64);
  if (d0 == 0) below = SGM_FAR;                                        // d - 1 < 0; the lane below belongs to another pixel
  if (d0 + SGM_PER_LANE >= D) above = SGM_FAR;                         // d + 1 >= D; likewise
  const int lo[SGM_PER_LANE] = {below, L[0], L[1], L[2]};
  const int hi[SGM_PER_LANE] = {L[1], L[2], L[3], above};              // an absent d + 1 inside the lane holds SGM_FAR already
#pragma unroll
  for (int k = 0; k < SGM_PER_LANE; ++k) {
    const int best = min(min(L[k], m + P2), min(lo[k], hi[k]) + P1);
    L[k] = (reset || d0 + k >= D) ? C[k] : C[k] + best - m;
  }
}

// S[d0 .. d0 + 3] = L, or += L, one 2-byte access each: the route of a D that is no multiple of four
template <bool ADD>
static __device__ inline void sgm_store(uint16_t* __restrict__ S, const int (&L)[SGM_PER_LANE], int d0, int D) {
#pragma unroll
  for (int k = 0; k < SGM_PER_LANE; ++k)
    if (d0 + k < D) S[d0 + k] = (uint16_t)((ADD ? S[d0 + k] : 0) + L[k]);
}

// One horizontal path over a row, DIR = +1 from the left or -1 from the right, SGM_ROW_CHUNK pixels at a time: everything a chunk
// reads from memory (the census words: a lane's four right words of neighbouring pixels overlap, so a chunk needs CHUNK + 3 of
// them; and, when adding, what S holds) is requested before its first step, so the loads of a chunk are in flight together and
// the dependent chain of the steps waits for memory once a chunk, not once a pixel.
template <int G, bool VEC, bool ADD, int DIR>
static __device__ inline void sgm_row_pass(const uint64_t* __restrict__ CL, const uint64_t* __restrict__ CR, uint16_t* __restrict__ S,
                                           int W, int D, int d0, int P1, int P2) {
  constexpr int U = SGM_ROW_CHUNK;
  int L[SGM_PER_LANE] = {SGM_FAR, SGM_FAR, SGM_FAR, SGM_FAR}, C[SGM_PER_LANE];
  const bool holds = d0 < D;                                           // lanes beyond D take part in the shuffles only
  for (int c = 0; c < W; c += U) {                                     // c: pixels walked so far; uniform over the launch
    const int xs = DIR > 0 ? c : W - 1 - c;                            // the chunk's first pixel in walking order
    const int lo = (DIR > 0 ? xs : xs - (U - 1)) - d0 - (SGM_PER_LANE - 1);      // the smallest right-word index of the chunk
    uint64_t l[U], r[U + SGM_PER_LANE - 1];
    sgm_u16x4 old[U];
#pragma unroll
    for (int i = 0; i < U + SGM_PER_LANE - 1; ++i) r[i] = (holds && lo + i >= 0 && lo + i < W) ? CR[lo + i] : 0;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int x = xs + DIR * u;
      const bool in = c + u < W;
      l[u] = in ? CL[x] : 0;
      old[u] = sgm_u16x4{0, 0, 0, 0};
      if (VEC && ADD && in && holds) old[u] = *(const sgm_u16x4*)(S + (long)x * D + d0);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (c + u >= W) break;                                           // uniform
      const int x = xs + DIR * u;
      // the word at x - d0 - k sits at r[x - d0 - k - lo]: u + 3 - k from the left, U + 2 - u - k from the right
      const int i0 = DIR > 0 ? u + SGM_PER_LANE - 1 : U + SGM_PER_LANE - 2 - u;
      sgm_cost(C, l[u], r[i0], r[i0 - 1], r[i0 - 2], r[i0 - 3], x, d0, D);
      sgm_step<G>(L, C, c + u == 0, d0, D, P1, P2);
      if (VEC) {
        if (holds) {
          sgm_u16x4 v = old[u];
          v.x += (unsigned short)L[0]; v.y += (unsigned short)L[1]; v.z += (unsigned short)L[2]; v.w += (unsigned short)L[3];
          *(sgm_u16x4*)(S + (long)x * D + d0) = v;
        }
      } else {
        sgm_store<ADD>(S + (long)x * D, L, d0, D);
      }
    }
  }
}

template <int G, bool VEC>
__global__ __launch_bounds__(SGM_BLOCK) void sgm_rows_kernel(SgmAggArgs a) {
  const int W = a.W, D = a.D;
  const int d0 = (threadIdx.x & (G - 1)) * SGM_PER_LANE;
  const long per_block = SGM_BLOCK / G;
  for (long line = blockIdx.x * per_block + threadIdx.x / G; line < a.lines; line += gridDim.x * per_block) {
    const uint64_t* CL = a.cl + line * W;
    const uint64_t* CR = a.cr + line * W;
    uint16_t* S = a.S + line * W * D;
    sgm_row_pass<G, VEC, false, +1>(CL, CR, S, W, D, d0, a.P1, a.P2);
    sgm_row_pass<G, VEC, true, -1>(CL, CR, S, W, D, d0, a.P1, a.P2);
  }
}

template <int G, bool VEC>
__global__ __launch_bounds__(SGM_BLOCK) void sgm_cols_kernel(SgmAggArgs a) {
  constexpr int U = SGM_COL_CHUNK;
  const int H = a.H, W = a.W, D = a.D, dy = a.dy, dx = a.dx;
  const int d0 = (threadIdx.x & (G - 1)) * SGM_PER_LANE;
  const bool holds = d0 < D;
  const long per_block = SGM_BLOCK / G;
  for (long line = blockIdx.x * per_block + threadIdx.x / G; line < a.lines; line += gridDim.x * per_block) {
    const long b = line / W;
    int x = (int)(line - b * W);                                        // the line's column in its first row
    int y = dy > 0 ? 0 : H - 1;
    const uint64_t* CL = a.cl + b * H * W;
    const uint64_t* CR = a.cr + b * H * W;
    uint16_t* S = a.S + b * H * W * D;
    int L[SGM_PER_LANE] = {SGM_FAR, SGM_FAR, SGM_FAR, SGM_FAR}, C[SGM_PER_LANE];
    for (int t = 0; t < H; t += U) {                                    // a chunk of the line: its loads first, as in sgm_row_pass
      int xs[U], ys[U];
      bool reset[U];
      uint64_t l[U], r[U][SGM_PER_LANE];
      sgm_u16x4 old[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        xs[u] = x; ys[u] = y;
        // the predecessor (y - dy, x - dx) lies outside the image: the first row, or x has just wrapped
        reset[u] = t + u == 0 || (dx > 0 && x == 0) || (dx < 0 && x == W - 1);
        const bool in = t + u < H;
        const long row = (long)y * W;
        l[u] = in ? CL[row + x] : 0;
#pragma unroll
        for (int k = 0; k < SGM_PER_LANE; ++k) r[u][k] = (in && d0 + k < D && x - d0 - k >= 0) ? CR[row + x - d0 - k] : 0;
        old[u] = sgm_u16x4{0, 0, 0, 0};
        if (VEC && in && holds) old[u] = *(const sgm_u16x4*)(S + (row + x) * D + d0);
        x += dx;
        x = x >= W ? 0 : x < 0 ? W - 1 : x;
        y += dy;                                                        // leaves the image after the line's last pixel: not used then
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (t + u >= H) break;                                          // uniform
        sgm_cost(C, l[u], r[u][0], r[u][1], r[u][2], r[u][3], xs[u], d0, D);
        sgm_step<G>(L, C, reset[u], d0, D, a.P1, a.P2);
        uint16_t* at = S + ((long)ys[u] * W + xs[u]) * D;
        if (VEC) {
          if (holds) {
            sgm_u16x4 v = old[u];
            v.x += (unsigned short)L[0]; v.y += (unsigned short)L[1]; v.z += (unsigned short)L[2]; v.w += (unsigned short)L[3];
            *(sgm_u16x4*)(at + d0) = v;
          }
        } else {
          sgm_store<true>(at, L, d0, D);
        }
      }
    }
  }
}

template <int G, bool VEC>
static void sgm_aggregate_launch(SgmAggArgs a, int B, int paths, hipStream_t st) {
  const int64_t per_block = SGM_BLOCK / G;
  auto grid = [&](int64_t lines) {
    const int64_t blocks = (lines + per_block - 1) / per_block;
    return dim3((unsigned)(blocks < (1 << 20) ? blocks : (1 << 20)));
  };
  a.lines = (long)B * a.H;
  a.dy = 0; a.dx = 1;
  hipLaunchKernelGGL((sgm_rows_kernel<G, VEC>), grid(a.lines), dim3(SGM_BLOCK), 0, st, a);
  a.lines = (long)B * a.W;
  static const int dirs[6][2] = {{1, 0}, {-1, 0}, {1, 1}, {1, -1}, {-1, 1}, {-1, -1}};
  for (int i = 0; i < (paths == 8 ? 6 : 2); ++i) {
    a.dy = dirs[i][0]; a.dx = dirs[i][1];
    hipLaunchKernelGGL((sgm_cols_kernel<G, VEC>), grid(a.lines), dim3(SGM_BLOCK), 0, st, a);
  }
}

// the group width of D: the smallest power of two of lanes that holds D disparities four to a lane
static inline int sgm_group(int D) {
  int g = 1;
  while (g * SGM_PER_LANE < D) g *= 2;
  return g;
}

#define SGM_DISPATCH(D, CALL)                             \
  do {                                                    \
    const bool vec_ = (D) % SGM_PER_LANE == 0;            \
    switch (sgm_group(D)) {                               \
      case 1: if (vec_) { CALL(1, true); } else { CALL(1, false); } break;    \
      case 2: if (vec_) { CALL(2, true); } else { CALL(2, false); } break;    \
      case 4: if (vec_) { CALL(4, true); } else { CALL(4, false); } break;    \
      case 8: if (vec_) { CALL(8, true); } else { CALL(8, false); } break;    \
      case 16: if (vec_) { CALL(16, true); } else { CALL(16, false); } break; \
      case 32: if (vec_) { CALL(32, true); } else { CALL(32, false); } break; \
      default: if (vec_) { CALL(64, true); } else { CALL(64, false); } break; \
    }                                                     \
  } while (0)

extern "C" int as_sgm_aggregate(const uint64_t* census_l, const uint64_t* census_r, int B, int H, int W, int D, int P1, int P2,
                                int paths, void* workspace, void* stream) {
  AS_CHECK_ARG(census_l && census_r && workspace, "as_sgm_aggregate: null pointer");
  if (int rc = sgm_check_volume("as_sgm_aggregate", B, H, W, D)) return rc;
  AS_CHECK_ARG(paths == 4 || paths == 8, "as_sgm_aggregate: paths %d outside {4, 8}", paths);
  AS_CHECK_ARG(P1 >= 0 && P2 >= P1 && P2 <= 255, "as_sgm_aggregate: penalties P1 %d, P2 %d: 0 <= P1 <= P2 <= 255 is required", P1, P2);
  AS_CHECK_ARG((((uintptr_t)census_l | (uintptr_t)census_r) & 7) == 0, "as_sgm_aggregate: the census maps must be 8-byte aligned");
  AS_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "as_sgm_aggregate: workspace must be 16-byte aligned");
  const int64_t n = (int64_t)B * H * W;
  const AsRange r[] = {{census_l, n * 8}, {census_r, n * 8}, {workspace, n * D * 2}};
  AS_CHECK_ARG(as_disjoint(r, 2, 3), "as_sgm_aggregate: workspace may not alias a census map (overlapping ranges)");
  SgmAggArgs a;
  a.cl = census_l; a.cr = census_r; a.S = (uint16_t*)workspace;
  a.H = H; a.W = W; a.D = D; a.P1 = P1; a.P2 = P2;
  a.lines = 0; a.dy = 0; a.dx = 0;
#define SGM_AGG_CALL(G, V) sgm_aggregate_launch<G, V>(a, B, paths, (hipStream_t)stream)
  SGM_DISPATCH(D, SGM_AGG_CALL);
#undef SGM_AGG_CALL
  AS_CHECK_LAUNCH("as_sgm_aggregate");
  return AS_OK;
}

// ------------------------------------------------------------------------------------------------ selection
struct SgmSelectArgs {
  const uint16_t* S;
  float* disp[2];
  uint8_t* code[2];
  int32_t* counts;
  int H, W, D, uniqueness;
  float fill;
};

static __device__ inline int sgm_pick4(const int (&s)[SGM_PER_LANE], int k) {
  return k == 0 ? s[0] : k == 1 ? s[1] : k == 2 ? s[2] : s[3];
}

// the winner of a column of n values held four to a lane over the group: -> d*, the sub-pixel value, whether it is not unique.
// Entries at or beyond n are ignored whatever they hold.  Every lane of the group returns the same.
template <int G>
static __device__ inline void sgm_winner(const int (&s)[SGM_PER_LANE], int d0, int n, int uniqueness, int& dstar, float& value,
                                         bool& ambiguous) {
  unsigned key = 0xFFFFFFFFu;
#pragma unroll
  for (int k = 0; k < SGM_PER_LANE; ++k)
    if (d0 + k < n) key = min(key, ((unsigned)s[k] << 9) | (unsigned)(d0 + k));          // equal values: the smallest d wins
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) key = min(key, (unsigned)__shfl_xor((int)key, o, 64));
  dstar = (int)(key & 511u);
  const int s1 = (int)(key >> 9);
  int bad = 0;
#pragma unroll
  for (int k = 0; k < SGM_PER_LANE; ++k) {
    const int d = d0 + k;
    bad |= d < n && (d < dstar - 1 || d > dstar + 1) && s[k] * (100 - uniqueness) < s1 * 100;
  }
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) bad |= __shfl_xor(bad, o, 64);
  ambiguous = bad != 0;
  // s[d* - 1] and s[d* + 1] from the lanes that hold them (indices clamped into the column: unused at its ends)
  const int first = (int)(threadIdx.x & 63) & ~(G - 1);
  const int im = max(dstar - 1, 0), ip = min(dstar + 1, n - 1);
  const int sm = __shfl(sgm_pick4(s, im & 3), first + (im >> 2), 64);
  const int sp = __shfl(sgm_pick4(s, ip & 3), first + (ip >> 2), 64);
  const int den = 2 * (sm + sp - 2 * s1);
  value = (float)dstar;
  if (dstar > 0 && dstar < n - 1 && den > 0) {
    const float off = (float)(sm - sp) / (float)den;
    value = (float)dstar + off;
  }
}

template <int G, bool VEC>
__global__ __launch_bounds__(SGM_BLOCK) void sgm_select_kernel(SgmSelectArgs a) {
  __shared__ int s_count[2 * SGM_CODES];
  as_counts_begin(s_count, 2 * SGM_CODES);
  const int W = a.W, D = a.D;
  const long pixels = (long)a.H * W;
  const long image = blockIdx.y * pixels;
  const uint16_t* S = a.S + image * D;
  const int j = threadIdx.x & (G - 1), d0 = j * SGM_PER_LANE;
  const long per_block = SGM_BLOCK / G;
  const bool want_right = a.disp[1] || a.code[1] || a.counts;
  const bool want_left = a.disp[0] || a.code[0] || a.counts;
  int mine[2][3] = {{0, 0, 0}, {0, 0, 0}};                             // per view: codes 0, 3, 7 (lane 0 of each group counts)
  // grid-stride over the pixels: at any moment the resident waves work on one window of consecutive pixels, so the lines the right
  // view's diagonal S(x + d, d) touches are shared between them in L2 (a run of pixels per wave instead was 2.8 x slower: measured)
  for (long p = blockIdx.x * per_block + threadIdx.x / G; p < pixels; p += gridDim.x * per_block) {
    const int x = (int)(p % W);
    for (int view = 0; view < 2; ++view) {
      if (!(view ? want_right : want_left)) continue;                  // uniform over the launch
      const int n = view ? min(D, W - x) : D;
      int s[SGM_PER_LANE];
      if (view == 0 && VEC) {
        sgm_u16x4 v = {0, 0, 0, 0};
        if (d0 < D) v = *(const sgm_u16x4*)(S + p * D + d0);
        s[0] = v.x; s[1] = v.y; s[2] = v.z; s[3] = v.w;
      } else {
#pragma unroll
        for (int k = 0; k < SGM_PER_LANE; ++k) {
          const int d = d0 + k;
          s[k] = d < n ? S[(p + (view ? d : 0)) * D + d] : 0;
        }
      }
      int dstar;
      float value;
      bool ambiguous;
      sgm_winner<G>(s, d0, n, a.uniqueness, dstar, value, ambiguous);
      const int code = (view == 0 && dstar > x) ? 3 : ambiguous ? 7 : 0;
      if (j == 0) {
        if (a.disp[view]) a.disp[view][image + p] = code == 0 ? value : a.fill;
        if (a.code[view]) a.code[view][image + p] = (uint8_t)code;
        mine[view][0] += code == 0;
        mine[view][1] += code == 3;
        mine[view][2] += code == 7;
      }
    }
  }
  if (a.counts == nullptr) return;                                     // uniform: no lane waits below
  const int slot[3] = {0, 3, 7};
#pragma unroll
  for (int view = 0; view < 2; ++view)
#pragma unroll
    for (int c = 0; c < 3; ++c) as_counts_add(&s_count[view * SGM_CODES + slot[c]], mine[view][c]);
  as_counts_flush(s_count, 2 * SGM_CODES, a.counts + blockIdx.y * 2 * SGM_CODES);
}

template <int G, bool VEC>
static void sgm_select_launch(const SgmSelectArgs& a, int B, hipStream_t st) {
  const int64_t blocks = as_div_up((int64_t)a.H * a.W, SGM_BLOCK / G);
  hipLaunchKernelGGL((sgm_select_kernel<G, VEC>), as_strided_grid(blocks, 4 * SGM_GROUPS, B), dim3(SGM_BLOCK), 0, st, a);
}

extern "C" int as_sgm_select(const void* workspace, int B, int H, int W, int D, int uniqueness, float fill, float* disp_l,
                             uint8_t* code_l, float* disp_r, uint8_t* code_r, int32_t* counts, void* stream) {
  AS_CHECK_ARG(workspace, "as_sgm_select: null pointer");
  if (int rc = sgm_check_volume("as_sgm_select", B, H, W, D)) return rc;
  AS_CHECK_ARG(uniqueness >= 0 && uniqueness <= 99, "as_sgm_select: uniqueness %d outside 0 .. 99", uniqueness);
  AS_CHECK_ARG(disp_l || code_l || disp_r || code_r || counts, "as_sgm_select: no output requested");
  AS_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "as_sgm_select: workspace must be 16-byte aligned");
  AS_CHECK_ARG((((uintptr_t)disp_l | (uintptr_t)disp_r | (uintptr_t)counts) & 3) == 0,
               "as_sgm_select: disp_l, disp_r and counts must be 4-byte aligned");
  const int64_t n = (int64_t)B * H * W;
  const AsRange r[] = {{workspace, n * D * 2}, {disp_l, n * 4}, {code_l, n}, {disp_r, n * 4}, {code_r, n},
                       {counts, (int64_t)B * 2 * SGM_CODES * 4}};
  AS_CHECK_ARG(as_disjoint(r, 1, 6), "as_sgm_select: an output may alias neither the workspace nor another output (overlapping ranges)");
  hipStream_t st = (hipStream_t)stream;
  if (int rc = as_clear_counts("as_sgm_select", counts, B * 2 * SGM_CODES, st)) return rc;
  SgmSelectArgs a;
  a.S = (const uint16_t*)workspace;
  a.disp[0] = disp_l; a.disp[1] = disp_r; a.code[0] = code_l; a.code[1] = code_r; a.counts = counts;
  a.H = H; a.W = W; a.D = D; a.uniqueness = uniqueness; a.fill = fill;
#define SGM_SEL_CALL(G, V) sgm_select_launch<G, V>(a, B, st)
  SGM_DISPATCH(D, SGM_SEL_CALL);
#undef SGM_SEL_CALL
  AS_CHECK_LAUNCH("as_sgm_select");
  return AS_OK;
}
