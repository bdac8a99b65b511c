// Colour-mapped disparity and error images on the device: the compute of the reference's utils/visualization.py (apply_cmap,
// visualize_disp_cv, visualize_disp_tensorboard, tensor_to_cv_rgb / _gray / _disp), which copies the map to the host, normalises
// it there and pushes every pixel through matplotlib's Colormap.__call__ (a float64 RGBA intermediate of 16 B/pixel).
//
// The arithmetic is a CONTRACT (include/adaptive_stereo_hip.h, restated by tests/visualization_ref.py):
//   v   = x, or |y - x| formed on the fly
//   n   = (v - lo) / den      one fp32 subtraction, one correctly rounded fp32 division (never a reciprocal: it moves pixels into the
//                             neighbouring bin); t = n * (float)N
//   idx = bad for NaN, N - 1 for t == N, under for t < 0, over for t > N, else (int)t
// lo and den come by value (both bounds fixed: one launch) or from the image's own minimum and maximum (two launches).
//
//   vis_range_kernel   grid (P, B): workgroup (j, b) reduces the j-th of P equal runs of image b to a (min, max) pair in the
//                      workspace.  Comparisons, never fminf / fmaxf: a NaN in the image is a NaN in both, as with torch.min.
//   vis_map_kernel     256 lanes x 4 pixels over the FLAT batch.  Prologue: the table goes to LDS, and wave w folds the P partials
//                      of image b0 + w (b0 = the image of the workgroup's first pixel) — no finalize launch.  A pixel of an image
//                      further on (images of fewer than 342 pixels) folds its own.  The range is resolved per pixel, so a dword that
//                      straddles two images carries each image's own colours.
//                      u8: a lane owns pixels 4g .. 4g+3 = bytes 12g .. 12g+11 = three whole dwords of the batch's byte stream
//                      (the base is 4-byte aligned, so there is no head); only the last lane peels a tail of byte stores.
//   vis_to_cv_kernel   the three conversions without a colour map, the same flat dword scheme over [B][H][W][C] bytes.
#include "as_common.h"

#pragma clang fp contract(off)

#define VIS_THREADS 256
#define VIS_PIX 4                       // pixels of a lane
#define VIS_BLOCK_PIX (VIS_THREADS * VIS_PIX)
#define VIS_MAX_PARTS 64                // partials of an image: one wave folds them
#define VIS_PART_PIXELS 4096
#define VIS_WAVES (VIS_THREADS / 64)    // images whose range the prologue folds
#define VIS_MAX_N 256
#define VIS_MAX_PIXELS ((int64_t)1 << 30)
#define VIS_MAX_BATCH 65535

enum { VIS_U8_RGB = 0, VIS_U8_BGR = 1, VIS_F32 = 2, VIS_INDEX = 3 };

// min / max that keep a NaN once they have met one (fminf, fmaxf and v_min_f32 drop it)
__device__ inline float vis_min(float m, float a) { return (a != a || a < m) ? a : m; }
__device__ inline float vis_max(float m, float a) { return (a != a || a > m) ? a : m; }
__device__ inline float vis_wave_min(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = vis_min(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ inline float vis_wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = vis_max(v, __shfl_xor(v, o, 64));
  return v;
}

static inline int vis_parts(int64_t HW) {
  const int64_t p = (HW + VIS_PART_PIXELS - 1) / VIS_PART_PIXELS;
  return (int)(p < 1 ? 1 : p > VIS_MAX_PARTS ? VIS_MAX_PARTS : p);
}

__global__ __launch_bounds__(VIS_THREADS) void vis_range_kernel(const float* __restrict__ x, const float* __restrict__ y, int HW,
                                                                int P, float* __restrict__ ws) {
  const int j = blockIdx.x, b = blockIdx.y;
  const int chunk = (HW + P - 1) / P;
  const int p0 = j * chunk;                                   // < HW + P: an empty run writes the identity (+inf, -inf)
  const int p1 = p0 + chunk < HW ? p0 + chunk : HW;
  const float* xb = x + (long)b * HW;
  const float* yb = y ? y + (long)b * HW : nullptr;
  float lo = INFINITY, hi = -INFINITY;
  for (int p = p0 + (int)threadIdx.x; p < p1; p += VIS_THREADS) {
    float v = xb[p];
    if (yb) v = fabsf(yb[p] - v);
    lo = vis_min(lo, v);
    hi = vis_max(hi, v);
  }
  __shared__ float part[2][VIS_WAVES];
  lo = vis_wave_min(lo);
  hi = vis_wave_max(hi);
  if ((threadIdx.x & 63) == 0) {
    part[0][threadIdx.x >> 6] = lo;
    part[1][threadIdx.x >> 6] = hi;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < VIS_WAVES; ++w) {
      lo = vis_min(lo, part[0][w]);
      hi = vis_max(hi, part[1][w]);
    }
    ws[2 * ((long)b * P + j)] = lo;
    ws[2 * ((long)b * P + j) + 1] = hi;
  }
}

// the table index of one value; N .. N + 2 are under, over, bad
__device__ inline int vis_index(float v, float lo, float den, int N) {
  const float n = (v - lo) / den;
  const float t = n * (float)N;
  if (t != t) return N + 2;
  if (t == (float)N) return N - 1;
  if (t < 0.f) return N;
  if (t > (float)N) return N + 1;
  return (int)t;
}

struct VisBounds {
  int automatic;            // bit 0: lo is the image's minimum, bit 1: hi is the image's maximum
  float lo, hi, den;        // automatic == 0: lo and den are used as given; else the fixed one of lo / hi, den = hi - lo
};

template <int MODE>
__global__ __launch_bounds__(VIS_THREADS) void vis_map_kernel(const float* __restrict__ x, const float* __restrict__ y, uint32_t total,
                                                              uint32_t HW, int B, VisBounds bd, const float* __restrict__ ws, int P,
                                                              const void* __restrict__ table, int N, int vec, void* __restrict__ out) {
  __shared__ uint32_t tab_u8[VIS_MAX_N + 3];
  __shared__ float tab_f[MODE == VIS_F32 ? 3 * (VIS_MAX_N + 3) : 1];
  __shared__ float r_lo[VIS_WAVES], r_den[VIS_WAVES];
  const uint32_t tid = threadIdx.x;
  const uint32_t base = blockIdx.x * (uint32_t)VIS_BLOCK_PIX;
  const uint32_t b0 = base / HW;

  if (MODE == VIS_U8_RGB || MODE == VIS_U8_BGR) {
    for (int i = tid; i < N + 3; i += VIS_THREADS) {
      const uint32_t e = ((const uint32_t*)table)[i];        // bytes r, g, b, (unused)
      tab_u8[i] = MODE == VIS_U8_BGR ? ((e >> 16) & 0xFFu) | (e & 0xFF00u) | ((e & 0xFFu) << 16) : (e & 0xFFFFFFu);
    }
  } else if (MODE == VIS_F32) {
    for (int i = tid; i < 3 * (N + 3); i += VIS_THREADS) tab_f[i] = ((const float*)table)[4 * (i / 3) + i % 3];
  }
  if (bd.automatic) {                                         // (uniform)
    const uint32_t bi = b0 + (tid >> 6);
    const int l = tid & 63;
    float mn = INFINITY, mx = -INFINITY;
    if (bi < (uint32_t)B && l < P) {
      mn = ws[2 * ((long)bi * P + l)];
      mx = ws[2 * ((long)bi * P + l) + 1];
    }
    mn = vis_wave_min(mn);
    mx = vis_wave_max(mx);
    if (l == 0) {
      const float lo = (bd.automatic & 1) ? mn : bd.lo;
      const float hi = (bd.automatic & 2) ? mx : bd.hi;
      r_lo[tid >> 6] = lo;
      r_den[tid >> 6] = hi - lo;
    }
  }
  __syncthreads();

  // this lane's pixels: consecutive for the byte stream, interleaved across the workgroup for the plane and index outputs
  uint32_t p[VIS_PIX];
  float v[VIS_PIX];
  const bool consecutive = MODE == VIS_U8_RGB || MODE == VIS_U8_BGR;
#pragma unroll
  for (int j = 0; j < VIS_PIX; ++j) p[j] = consecutive ? base + tid * VIS_PIX + j : base + j * VIS_THREADS + tid;
  if (consecutive && vec && p[VIS_PIX - 1] < total) {
    const f32x4 a = *(const f32x4*)(x + p[0]);
#pragma unroll
    for (int j = 0; j < VIS_PIX; ++j) v[j] = a[j];
    if (y) {
      const f32x4 c = *(const f32x4*)(y + p[0]);
#pragma unroll
      for (int j = 0; j < VIS_PIX; ++j) v[j] = fabsf(c[j] - v[j]);
    }
  } else {
#pragma unroll
    for (int j = 0; j < VIS_PIX; ++j) {
      v[j] = 0.f;
      if (p[j] < total) {
        v[j] = x[p[j]];
        if (y) v[j] = fabsf(y[p[j]] - v[j]);
      }
    }
  }

  int idx[VIS_PIX];
#pragma unroll
  for (int j = 0; j < VIS_PIX; ++j) {
    float lo = bd.lo, den = bd.den;
    if (bd.automatic && p[j] < total) {
      const uint32_t b = p[j] / HW;
      if (b - b0 < VIS_WAVES) {
        lo = r_lo[b - b0];
        den = r_den[b - b0];
      } else {                                                // an image beyond the prologue's: fold its partials here
        float mn = INFINITY, mx = -INFINITY;
        for (int i = 0; i < P; ++i) {
          mn = vis_min(mn, ws[2 * ((long)b * P + i)]);
          mx = vis_max(mx, ws[2 * ((long)b * P + i) + 1]);
        }
        lo = (bd.automatic & 1) ? mn : bd.lo;
        den = ((bd.automatic & 2) ? mx : bd.hi) - lo;
      }
    }
    idx[j] = vis_index(v[j], lo, den, N);
  }

  if (consecutive) {
    if (p[VIS_PIX - 1] < total) {
      const uint32_t c0 = tab_u8[idx[0]], c1 = tab_u8[idx[1]], c2 = tab_u8[idx[2]], c3 = tab_u8[idx[3]];
      uint32_t* o = (uint32_t*)out + (size_t)(p[0] / VIS_PIX) * 3;
      o[0] = c0 | (c1 << 24);                                 // r0 g0 b0 r1
      o[1] = (c1 >> 8) | (c2 << 16);                          // g1 b1 r2 g2
      o[2] = (c2 >> 16) | (c3 << 8);                          // b2 r3 g3 b3
    } else {
      uint8_t* o = (uint8_t*)out;
#pragma unroll
      for (int j = 0; j < VIS_PIX; ++j) {
        if (p[j] < total) {
          const uint32_t c = tab_u8[idx[j]];
          o[(size_t)p[j] * 3] = (uint8_t)c;
          o[(size_t)p[j] * 3 + 1] = (uint8_t)(c >> 8);
          o[(size_t)p[j] * 3 + 2] = (uint8_t)(c >> 16);
        }
      }
    }
  } else if (MODE == VIS_F32) {
    float* o = (float*)out;
#pragma unroll
    for (int j = 0; j < VIS_PIX; ++j) {
      if (p[j] < total) {
        const uint32_t b = p[j] / HW, pix = p[j] - b * HW;
        float* ob = o + (size_t)b * 3 * HW + pix;
        ob[0] = tab_f[3 * idx[j]];
        ob[HW] = tab_f[3 * idx[j] + 1];
        ob[2 * (size_t)HW] = tab_f[3 * idx[j] + 2];
      }
    }
  } else {
    int16_t* o = (int16_t*)out;
#pragma unroll
    for (int j = 0; j < VIS_PIX; ++j)
      if (p[j] < total) o[p[j]] = (int16_t)idx[j];
  }
}

static int vis_check_shape(const char* who, int B, int H, int W) {
  AS_CHECK_ARG(B > 0 && H > 0 && W > 0, "%s: B %d, H %d and W %d must be positive", who, B, H, W);
  AS_CHECK_ARG(B <= VIS_MAX_BATCH && (int64_t)B * H * W <= VIS_MAX_PIXELS, "%s: B %d of at most %d, B*H*W %lld of at most 2^30", who, B,
               VIS_MAX_BATCH, (long long)((int64_t)B * H * W));
  return AS_OK;
}

extern "C" int64_t as_colormap_workspace(int B, int64_t pixels_per_image) {
  if (B <= 0 || B > VIS_MAX_BATCH || pixels_per_image <= 0 || pixels_per_image > VIS_MAX_PIXELS / B) return -1;
  return (int64_t)B * vis_parts(pixels_per_image) * 2 * (int64_t)sizeof(float);
}

extern "C" int as_colormap_range(const float* x, const float* y, int B, int H, int W, void* workspace, void* stream) {
  AS_CHECK_ARG(x && workspace, "as_colormap_range: x and workspace must not be NULL");
  if (int rc = vis_check_shape("as_colormap_range", B, H, W)) return rc;
  AS_CHECK_ARG(((uintptr_t)workspace & 3) == 0, "as_colormap_range: workspace must be 4-byte aligned");
  const int HW = H * W, P = vis_parts(HW);
  hipLaunchKernelGGL(vis_range_kernel, dim3(P, B), dim3(VIS_THREADS), 0, (hipStream_t)stream, x, y, HW, P, (float*)workspace);
  AS_CHECK_LAUNCH("as_colormap_range");
  return AS_OK;
}

extern "C" int as_colormap_apply(const float* x, const float* y, int B, int H, int W, int automatic, float lo, float hi, float den,
                                 const void* workspace, const void* table, int N, int mode, void* out, void* stream) {
  AS_CHECK_ARG(x && out, "as_colormap_apply: x and out must not be NULL");
  if (int rc = vis_check_shape("as_colormap_apply", B, H, W)) return rc;
  AS_CHECK_ARG(N >= 1 && N <= VIS_MAX_N, "as_colormap_apply: N %d outside [1, %d]", N, VIS_MAX_N);
  AS_CHECK_ARG(mode >= VIS_U8_RGB && mode <= VIS_INDEX, "as_colormap_apply: mode %d (0 u8 RGB, 1 u8 BGR, 2 f32, 3 index)", mode);
  AS_CHECK_ARG(automatic >= 0 && automatic <= 3, "as_colormap_apply: automatic %d is not a mask of bits 0 and 1", automatic);
  AS_CHECK_ARG(!automatic || workspace, "as_colormap_apply: an automatic bound needs the workspace of as_colormap_range");
  AS_CHECK_ARG(mode == VIS_INDEX || table, "as_colormap_apply: table must not be NULL for a colour output");
  AS_CHECK_ARG(((uintptr_t)table & 3) == 0, "as_colormap_apply: table must be 4-byte aligned");
  const uintptr_t align = mode == VIS_INDEX ? 1 : 3;
  AS_CHECK_ARG(((uintptr_t)out & align) == 0, "as_colormap_apply: out must be %d-byte aligned for mode %d", (int)align + 1, mode);
  AS_CHECK_ARG(((uintptr_t)x & 3) == 0 && ((uintptr_t)y & 3) == 0, "as_colormap_apply: x and y must be 4-byte aligned");
  const uint32_t HW = (uint32_t)H * W, total = (uint32_t)B * HW;
  const int P = vis_parts(HW);
  const int vec = (((uintptr_t)x | (uintptr_t)y) & 15) == 0;
  VisBounds bd;
  bd.automatic = automatic; bd.lo = lo; bd.hi = hi; bd.den = den;
  const dim3 grid(as_div_up(total, VIS_BLOCK_PIX)), block(VIS_THREADS);
  hipStream_t st = (hipStream_t)stream;
  const float* ws = (const float*)workspace;
  switch (mode) {
    case VIS_U8_RGB:
      hipLaunchKernelGGL(vis_map_kernel<VIS_U8_RGB>, grid, block, 0, st, x, y, total, HW, B, bd, ws, P, table, N, vec, out);
      break;
    case VIS_U8_BGR:
      hipLaunchKernelGGL(vis_map_kernel<VIS_U8_BGR>, grid, block, 0, st, x, y, total, HW, B, bd, ws, P, table, N, vec, out);
      break;
    case VIS_F32:
      hipLaunchKernelGGL(vis_map_kernel<VIS_F32>, grid, block, 0, st, x, y, total, HW, B, bd, ws, P, table, N, vec, out);
      break;
    default:
      hipLaunchKernelGGL(vis_map_kernel<VIS_INDEX>, grid, block, 0, st, x, y, total, HW, B, bd, ws, P, table, N, vec, out);
  }
  AS_CHECK_LAUNCH("as_colormap_apply");
  return AS_OK;
}

// ---- conversions without a colour map ---------------------------------------------------------------------------------------
// in [B][C][H][W] fp32 -> out [B][H][W][C]; element e of the flat output is t = 255.0f * v, then t / div when div != 0 (two
// separately rounded operations), saturated to 0 .. 255 and truncated for the uint8 output (a NaN is 0).
template <int C>
__global__ __launch_bounds__(VIS_THREADS) void vis_to_cv_kernel(const float* __restrict__ in, uint32_t total, uint32_t HW, int flip,
                                                                float div, int out_f32, void* __restrict__ out) {
  const uint32_t e0 = (blockIdx.x * (uint32_t)VIS_THREADS + threadIdx.x) * 4u;
  float t[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    t[j] = 0.f;
    const uint32_t e = e0 + j;
    if (e < total) {
      const uint32_t q = e / C, c = e - q * C;
      const uint32_t b = q / HW, pix = q - b * HW;
      const uint32_t cs = flip ? C - 1 - c : c;
      t[j] = 255.0f * in[((size_t)b * C + cs) * HW + pix];
      if (div != 0.f) t[j] = t[j] / div;
    }
  }
  if (out_f32) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (e0 + j < total) ((float*)out)[e0 + j] = t[j];
    return;
  }
  uint32_t u[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) u[j] = t[j] >= 255.f ? 255u : t[j] > 0.f ? (uint32_t)t[j] : 0u;
  if (e0 + 3 < total) {
    ((uint32_t*)out)[e0 >> 2] = u[0] | (u[1] << 8) | (u[2] << 16) | (u[3] << 24);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (e0 + j < total) ((uint8_t*)out)[e0 + j] = (uint8_t)u[j];
  }
}

extern "C" int as_image_to_cv(const float* in, int B, int C, int H, int W, int flip, float div, int out_f32, void* out, void* stream) {
  AS_CHECK_ARG(in && out, "as_image_to_cv: in and out must not be NULL");
  if (int rc = vis_check_shape("as_image_to_cv", B, H, W)) return rc;
  AS_CHECK_ARG(C == 1 || C == 3, "as_image_to_cv: C %d (1 or 3)", C);
  AS_CHECK_ARG((int64_t)B * H * W * C <= VIS_MAX_PIXELS, "as_image_to_cv: B*H*W*C beyond 2^30");
  AS_CHECK_ARG(((uintptr_t)out & 3) == 0 && ((uintptr_t)in & 3) == 0, "as_image_to_cv: in and out must be 4-byte aligned");
  AS_CHECK_ARG(div == div && div >= 0.f, "as_image_to_cv: div %g must be >= 0 (0: no division)", (double)div);
  const uint32_t HW = (uint32_t)H * W, total = (uint32_t)B * HW * C;
  const dim3 grid(as_div_up(total, VIS_THREADS * 4)), block(VIS_THREADS);
  if (C == 1)
    hipLaunchKernelGGL(vis_to_cv_kernel<1>, grid, block, 0, (hipStream_t)stream, in, total, HW, flip, div, out_f32, out);
  else
    hipLaunchKernelGGL(vis_to_cv_kernel<3>, grid, block, 0, (hipStream_t)stream, in, total, HW, flip, div, out_f32, out);
  AS_CHECK_LAUNCH("as_image_to_cv");
  return AS_OK;
}
