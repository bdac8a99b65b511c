// Edge-aware smoothing of a full-resolution disparity map: the image-guided weighted median (Ma et al., ICCV 2013), whose
// uniform-weight case is the plain median every classical pipeline ends in.  A CONTRACT (include/adaptive_stereo_hip.h, restated
// in numpy by tests/disp_smooth_ref.py): the output is always one of the inputs (a selected float) and every weight an integer, so
// the result is a pure function of the input.
//
// Geometry: a workgroup of DS_LANES = 256 lanes owns a tile of DS_ROWS = 16 rows x DS_SPAN = 64 columns and strides over the tiles
// of one image; grid (about DS_GROUPS / B, B).  It stages the tile and a halo of `radius` once in LDS, two 32-bit words a pixel:
//   s_key   the disparity's bits where the pixel is a tap (in the image and usable), DS_NOT_A_TAP elsewhere
//   s_gd    the guide quantised to 8 bits a channel, packed (guided launches only)
// and the clamped weight table beside them.  A wave then takes the tile's rows wave, wave + 4, ..., one lane a pixel.
//
// Selection without a sort, by bisection on the int32 key that snaps to the window's own values:
//   pass 0     n, Wt and the window's smallest and largest key [lo, hi]
//   pass k     t = the midpoint of [lo, hi]; the weight of the taps with key <= t, the largest key <= t (below) and the smallest
//              key > t (above).  2 * weight >= Wt: the median is <= t, hi = below; else lo = above.  Both ends stay keys of the
//              window, the interval loses at least one of them a pass, and lo == hi is the median.
// A pass reads every word of the window once (two words and one table entry when guided): LDS reads a pixel = (1 + passes) x taps
// x (1 or 3).  The passes are at most 32 and about log2 of the window's distinct values for values spread evenly.
// DS_NOT_A_TAP (INT_MAX, a NaN's bits) lies above every key of a usable value, so no pass after pass 0 has to test for it: it is
// never <= t, and never the smallest key above t while hi is.
//
// A second route for the plain median of 9 or 25 taps (no guide, radius <= DS_NETWORK_RADIUS): the window is read once into
// registers, sorted by sort_net.h's fixed network (28 and 140 comparators, a max and a min each) and element (n - 1) / 2 taken.  Every
// (radius, guided) pair has exactly one route; both obey the one contract and the tests run both on the same inputs.
#include "code_maps.h"
#include "sort_net.h"

#pragma clang fp contract(off)

#define DS_SPAN 64                  // columns of a workgroup's tile; tests/disp_smooth_ref.py places its shapes by DS_SPAN and
#define DS_ROWS 16                  // DS_ROWS: change them there together with these
#define DS_LANES 256
#define DS_MAX_RADIUS 7
#define DS_LUT 768                  // entries of the weight table: the sums of 3 absolute differences of 8-bit values, and 2 spare
#define DS_COUNTS 4                 // usable and unchanged, usable and changed, filled, still rejected
#define DS_GROUPS 2048
#define DS_NOT_A_TAP 0x7FFFFFFF
#define DS_NETWORK_RADIUS 2          // the plain median up to this radius sorts its 9 or 25 taps in registers

struct DsArgs {
  const float* disp;
  const uint8_t* code_in;
  const float* guide;
  const int32_t* lut;
  float* out;
  uint8_t* code;
  int32_t* counts;
  int C, H, W, xblocks, fill, min_support;
};

// the contract's 8-bit guide: a NaN becomes 0 (fmaxf), values outside [0, 1] the nearest end
static __device__ inline unsigned ds_quantise(float v) {
  const float c = fminf(fmaxf(v, 0.f), 1.f);
  const float s = c * 255.f;
  return (unsigned)(int)rintf(s);
}

template <int R, bool GUIDED>
__global__ __launch_bounds__(DS_LANES) void disp_wmedian_kernel(DsArgs a) {
  constexpr int SW = DS_SPAN + 2 * R, SH = DS_ROWS + 2 * R, SIDE = 2 * R + 1;
  constexpr int ROWS_UNROLLED = R <= 2 ? SIDE : 1;                    // a small window whole; a large one row by row
  constexpr bool NETWORK = !GUIDED && R <= DS_NETWORK_RADIUS;
  __shared__ int s_key[SH * SW];
  __shared__ unsigned s_gd[GUIDED ? SH * SW : 1];
  __shared__ int s_lut[GUIDED ? DS_LUT : 1];
  __shared__ int s_count[DS_COUNTS];
  as_counts_begin(s_count, DS_COUNTS);
  const int H = a.H, W = a.W;
  const long plane = (long)H * W;
  const long image = (long)blockIdx.y * plane;
  const float* D = a.disp + image;
  const uint8_t* K = a.code_in ? a.code_in + image : nullptr;
  const float* G = GUIDED ? a.guide + image * a.C : nullptr;
  if (GUIDED)
    for (int i = threadIdx.x; i < DS_LUT; i += DS_LANES) s_lut[i] = min(max(a.lut[i], 0), 65535);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int mine[DS_COUNTS] = {0, 0, 0, 0};
  const long tiles = (long)((H + DS_ROWS - 1) / DS_ROWS) * a.xblocks;
  for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int ty = (int)(tile / a.xblocks);
    const int y0 = ty * DS_ROWS, x0 = (int)(tile - (long)ty * a.xblocks) * DS_SPAN;
    __syncthreads();                                                   // the previous tile's readers are done (and s_lut is in)
    for (int i = threadIdx.x; i < SH * SW; i += DS_LANES) {
      const int sy = i / SW, sx = i - sy * SW;
      const int y = y0 - R + sy, x = x0 - R + sx;
      int key = DS_NOT_A_TAP;
      unsigned g = 0;
      if (y >= 0 && y < H && x >= 0 && x < W) {
        const long at = (long)y * W + x;
        const float d = D[at];
        if ((K == nullptr || K[at] == 0) && as_disp_usable(d)) key = __float_as_int(d);
        if (GUIDED)
          for (int c = 0; c < a.C; ++c) g |= ds_quantise(G[c * plane + at]) << (8 * c);
      }
      s_key[i] = key;
      if (GUIDED) s_gd[i] = g;
    }
    __syncthreads();
    for (int ry = wave; ry < DS_ROWS; ry += DS_LANES / 64) {
      const int y = y0 + ry, x = x0 + lane;
      if (y >= H || x >= W) continue;
      const int corner = ry * SW + lane;                               // the window's first slot; the centre is R rows and columns on
      const int centre = corner + R * SW + R;
      const bool us = s_key[centre] != DS_NOT_A_TAP;
      int n = 0, wt = 0, lo = DS_NOT_A_TAP, hi = (int)0x80000000;
      bool select;
      if constexpr (NETWORK) {
        // ~key in DESCENDING order is the key in rising order with DS_NOT_A_TAP (~ = INT_MIN) behind every tap
        int v[SIDE * SIDE];
#pragma unroll
        for (int dy = 0; dy < SIDE; ++dy) {
#pragma unroll
          for (int dx = 0; dx < SIDE; ++dx) {
            const int k = s_key[corner + dy * SW + dx];
            n += k != DS_NOT_A_TAP;
            v[dy * SIDE + dx] = ~k;
          }
        }
        constexpr SortNet<SIDE * SIDE> net = make_sort_net<SIDE * SIDE>();
#pragma unroll
        for (int k = 0; k < net.n; ++k) {
          const int x_ = v[net.a[k]], y_ = v[net.b[k]];
          v[net.a[k]] = max(x_, y_);
          v[net.b[k]] = min(x_, y_);
        }
        const int rank = (n - 1) >> 1;                                 // every weight 1: the lower median of n taps
        int m = v[0];
#pragma unroll
        for (int j = 1; j < SIDE * SIDE; ++j) m = rank == j ? v[j] : m;
        wt = n;
        lo = ~m;
        select = wt > 0 && (us || (a.fill && n >= a.min_support));
      } else {
        const unsigned gp = GUIDED ? s_gd[centre] : 0u;
#pragma unroll ROWS_UNROLLED
        for (int dy = 0; dy < SIDE; ++dy) {
#pragma unroll
          for (int dx = 0; dx < SIDE; ++dx) {
            const int q = corner + dy * SW + dx;
            const int k = s_key[q];
            const bool tap = k != DS_NOT_A_TAP;
            const int w = GUIDED ? s_lut[__builtin_amdgcn_sad_u8(gp, s_gd[q], 0u)] : 1;
            n += tap;
            wt += tap ? w : 0;
            lo = min(lo, k);
            hi = tap ? max(hi, k) : hi;
          }
        }
        select = wt > 0 && (us || (a.fill && n >= a.min_support));
        if (!select) hi = lo;
        while (lo < hi) {
          const int t = lo + (int)(((unsigned)hi - (unsigned)lo) >> 1);
          int cum = 0, below = lo, above = hi;
#pragma unroll ROWS_UNROLLED
          for (int dy = 0; dy < SIDE; ++dy) {
#pragma unroll
            for (int dx = 0; dx < SIDE; ++dx) {
              const int q = corner + dy * SW + dx;
              const int k = s_key[q];
              const bool le = k <= t;
              const int w = GUIDED ? s_lut[__builtin_amdgcn_sad_u8(gp, s_gd[q], 0u)] : 1;
              cum += le ? w : 0;
              below = le ? max(below, k) : below;
              above = le ? above : min(above, k);
            }
          }
          if (2 * cum >= wt) hi = below; else lo = above;
        }
      }
      const long at = (long)y * W + x;
      const int own = __float_as_int(D[at]);                           // bits, so that a NaN keeps its payload
      const int cin = K ? K[at] : 0;
      const int bits = select ? lo : own;
      const int code = select ? 0 : us ? 0 : cin != 0 ? cin : 4;
      reinterpret_cast<int*>(a.out)[image + at] = bits;
      if (a.code) a.code[image + at] = (uint8_t)code;
      const int slot = us ? (bits != own) : select ? 2 : 3;
#pragma unroll
      for (int c = 0; c < DS_COUNTS; ++c) mine[c] += slot == c;
    }
  }
  if (a.counts == nullptr) return;                                     // uniform: no lane waits below
#pragma unroll
  for (int c = 0; c < DS_COUNTS; ++c) as_counts_add(&s_count[c], mine[c]);
  as_counts_flush(s_count, DS_COUNTS, a.counts + blockIdx.y * DS_COUNTS);
}

template <int R>
static void ds_launch(bool guided, dim3 grid, hipStream_t st, const DsArgs& a) {
  if (guided) hipLaunchKernelGGL((disp_wmedian_kernel<R, true>), grid, dim3(DS_LANES), 0, st, a);
  else hipLaunchKernelGGL((disp_wmedian_kernel<R, false>), grid, dim3(DS_LANES), 0, st, a);
}

extern "C" int as_disp_wmedian(const float* disp, const uint8_t* code_in, const float* guide, int C, const int32_t* weight_lut,
                               int B, int H, int W, int radius, int fill, int min_support, float* out, uint8_t* code,
                               int32_t* counts, void* stream) {
  AS_CHECK_ARG(disp && out, "as_disp_wmedian: null pointer");
  if (int rc = as_check_images("as_disp_wmedian", B, H, W, true)) return rc;
  AS_CHECK_ARG(!guide || C == 1 || C == 3, "as_disp_wmedian: C %d of the guide must be 1 or 3", C);
  AS_CHECK_ARG((guide != nullptr) == (weight_lut != nullptr),
               "as_disp_wmedian: a guide needs a weight table and a weight table a guide (both or neither)");
  AS_CHECK_ARG(radius >= 1 && radius <= DS_MAX_RADIUS, "as_disp_wmedian: radius %d must be 1 .. %d", radius, DS_MAX_RADIUS);
  AS_CHECK_ARG(fill == 0 || fill == 1, "as_disp_wmedian: fill %d must be 0 or 1", fill);
  AS_CHECK_ARG(min_support >= 1, "as_disp_wmedian: min_support %d must be at least 1", min_support);
  AS_CHECK_ARG((((uintptr_t)disp | (uintptr_t)guide | (uintptr_t)weight_lut | (uintptr_t)out | (uintptr_t)counts) & 3) == 0,
               "as_disp_wmedian: disp, guide, weight_lut, out and counts must be 4-byte aligned");
  const int64_t n = (int64_t)B * H * W;
  const AsRange r[] = {{disp, n * 4}, {code_in, n}, {guide, n * C * 4}, {weight_lut, DS_LUT * 4},
                       {out, n * 4}, {code, n}, {counts, (int64_t)B * DS_COUNTS * 4}};
  AS_CHECK_ARG(as_disjoint(r, 4, 7), "as_disp_wmedian: an output may alias neither an input nor another output (overlapping ranges)");
  hipStream_t st = (hipStream_t)stream;
  if (int rc = as_clear_counts("as_disp_wmedian", counts, B * DS_COUNTS, st)) return rc;
  DsArgs a;
  a.disp = disp; a.code_in = code_in; a.guide = guide; a.lut = weight_lut; a.out = out; a.code = code; a.counts = counts;
  a.C = guide ? C : 0; a.H = H; a.W = W; a.xblocks = as_div_up(W, DS_SPAN); a.fill = fill; a.min_support = min_support;
  const dim3 grid = as_strided_grid((int64_t)as_div_up(H, DS_ROWS) * a.xblocks, DS_GROUPS, B);
  const bool guided = guide != nullptr;
  switch (radius) {
    case 1: ds_launch<1>(guided, grid, st, a); break;
    case 2: ds_launch<2>(guided, grid, st, a); break;
    case 3: ds_launch<3>(guided, grid, st, a); break;
    case 4: ds_launch<4>(guided, grid, st, a); break;
    case 5: ds_launch<5>(guided, grid, st, a); break;
    case 6: ds_launch<6>(guided, grid, st, a); break;
    default: ds_launch<7>(guided, grid, st, a); break;
  }
  AS_CHECK_LAUNCH("as_disp_wmedian");
  return AS_OK;
}
