// Velodyne scan -> sparse ground-truth depth and disparity on the device: the compute of the reference's
// scripts/export_gt_disp.py (generate_depth_map :86-115, the conversion to disparity and to uint16 = 128 * disp :156-162), which
// the reference runs on the host with numpy and a Python loop per duplicated pixel.
//
// The arithmetic is a CONTRACT (include/adaptive_stereo_hip.h, restated op for op by tests/lidar_ref.py): the projection is
// fp64 on purpose, every expression a sequence of single IEEE operations in the written order, so nothing here may contract
// into an fma: a point has to land in the pixel the reference's float64 np.dot puts it in.
//
//   lidar_project_kernel   one lane per point (16 bytes each), lanes at or beyond counts[b] exit: x >= 0, q = P . (x, y, z, 1),
//                          u, v by round-half-even, bounds, then one atomicMin of the order-preserving key of the value into
//                          zbuf[b][v][u].  An integer minimum does not depend on arrival order.
//   lidar_resolve_kernel   one lane per pixel of the WHOLE buffer: every key read is handed back empty, so the next frame
//                          starts clean; inside the window depth, disparity, uint16 = 128 * disp and, with a prediction, the
//                          six sums of as_eval_metrics as per-block fp64 partials (no float atomics).
//   lidar_metrics_kernel   one wave per image adds the partials in a fixed order.
#include "as_common.h"

#pragma clang fp contract(off)

#define LD_EMPTY 0xFFFFFFFFu
#define LD_MAX_BATCH 65535            // images are the grid's y dimension
#define LD_MAX_PIXELS ((int64_t)1 << 30)

typedef unsigned long long u64;

// fp32 -> uint32 whose unsigned order is the order of the floats: the sign bit of a positive value is flipped, every bit of a
// negative one (-0.0 sorts just below +0.0).  No value maps to LD_EMPTY: that would be a NaN, and no NaN gets here.
__device__ inline uint32_t ld_encode(float v) {
  const uint32_t b = __float_as_uint(v);
  return (b & 0x80000000u) ? ~b : (b ^ 0x80000000u);
}
__device__ inline float ld_decode(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

__global__ __launch_bounds__(256) void lidar_project_kernel(const f32x4* __restrict__ points, const int* __restrict__ counts,
                                                            const double* __restrict__ P, int Nmax, int H, int W, int vel_depth,
                                                            uint32_t* __restrict__ zbuf) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int cnt = counts[b];
  if (i >= (cnt < Nmax ? cnt : Nmax)) return;           // also a negative count: nothing is read
  const f32x4 p = points[(long)b * Nmax + i];           // the fourth word (reflectance) is ignored: the point is (x, y, z, 1)
  if (!(p.x >= 0.f)) return;                            // keeps -0.0, drops NaN
  const double* M = P + b * 12;
  const double x = (double)p.x, y = (double)p.y, z = (double)p.z;
  const double q0 = ((M[0] * x + M[1] * y) + M[2] * z) + M[3];
  const double q1 = ((M[4] * x + M[5] * y) + M[6] * z) + M[7];
  const double q2 = ((M[8] * x + M[9] * y) + M[10] * z) + M[11];
  const double u = rint(q0 / q2) - 1.0, v = rint(q1 / q2) - 1.0;      // no test of q2 > 0; inf and NaN fail the comparisons below
  if (!(u >= 0.0 && u < (double)W && v >= 0.0 && v < (double)H)) return;
  const float value = vel_depth ? p.x : (float)q2;
  atomicMin(zbuf + ((long)b * H + (int)v) * W + (int)u, ld_encode(value));
}

__global__ __launch_bounds__(256) void lidar_resolve_kernel(uint32_t* __restrict__ zbuf, int H, int W, int i0, int j0, int h, int w,
                                                            double bf, int quantize, float* __restrict__ depth_out,
                                                            float* __restrict__ disp_out, uint16_t* __restrict__ disp_u16,
                                                            const float* __restrict__ pred, double* __restrict__ partial,
                                                            int* __restrict__ overflow) {
  __shared__ double red[6][4];
  const int b = blockIdx.y;
  const int hw = H * W;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const bool live = idx < hw;                           // no early return: the wave stays whole for the ballot and the sums
  uint32_t key = LD_EMPTY;
  if (live) {
    uint32_t* slot = zbuf + (long)b * hw + idx;
    key = *slot;
    if (key != LD_EMPTY) *slot = LD_EMPTY;              // hand the pixel back empty, inside the window or not
  }
  const int row = live ? idx / W : 0;
  const int r = row - i0, c = idx - row * W - j0;
  const bool inside = live && r >= 0 && r < h && c >= 0 && c < w;

  float depth = key == LD_EMPTY ? 0.f : ld_decode(key);
  depth = depth < 0.f ? 0.f : depth;
  double disp64 = bf / (double)depth;
  if (depth == 0.f || depth > 80.f) disp64 = 0.0;
  const double scaled = 128.0 * disp64;
  const bool over = inside && scaled > 65535.0;
  if (over) depth = 0.f;
  const uint32_t q = over ? 0u : (uint32_t)scaled;      // truncation; 0 <= scaled <= 65535 here
  const float disp = quantize ? (float)q / 128.f : (over ? 0.f : (float)disp64);

  const long out = ((long)b * h + r) * w + c;
  if (inside) {
    if (depth_out) depth_out[out] = depth;
    if (disp_out) disp_out[out] = disp;
    if (disp_u16) disp_u16[out] = (uint16_t)q;
  }
  if (overflow) {                                       // (uniform)  one integer add per wave: exact in any order
    const u64 mask = __ballot(over);
    if (mask && (threadIdx.x & 63) == __ffsll((long long)mask) - 1) atomicAdd(overflow + b, (int)__popcll(mask));
  }
  if (!pred) return;                                    // (uniform)

  double s[6] = {0, 0, 0, 0, 0, 0};
  if (inside && disp > 0.f) {                           // as eval_metrics_kernel: strict >, fp32 error
    const float e = fabsf(pred[out] - disp);
    s[0] = (double)e; s[1] = 1.0;
    s[2] = e > 2.f ? 1.0 : 0.0; s[3] = e > 3.f ? 1.0 : 0.0;
    s[4] = e > 4.f ? 1.0 : 0.0; s[5] = e > 5.f ? 1.0 : 0.0;
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    s[k] = wave_sum_d(s[k]);
    if ((threadIdx.x & 63) == 0) red[k][threadIdx.x >> 6] = s[k];
  }
  __syncthreads();
  if (threadIdx.x < 6)
    partial[((long)b * gridDim.x + blockIdx.x) * 6 + threadIdx.x] =
        ((red[threadIdx.x][0] + red[threadIdx.x][1]) + red[threadIdx.x][2]) + red[threadIdx.x][3];
}

// one wave per image: lane t adds blocks t, t + 64, ... in order, then the xor butterfly
__global__ __launch_bounds__(64) void lidar_metrics_kernel(const double* __restrict__ partial, int nblk, float* __restrict__ metrics) {
  const int b = blockIdx.x;
  for (int m = 0; m < 6; ++m) {
    double s = 0.0;
    for (int i = threadIdx.x; i < nblk; i += 64) s += partial[((long)b * nblk + i) * 6 + m];
    s = wave_sum_d(s);
    if (threadIdx.x == 0) metrics[b * 6 + m] = (float)s;
  }
}

static bool ld_frame_ok(int B, int H, int W) {
  return B > 0 && B <= LD_MAX_BATCH && H > 0 && W > 0 && (int64_t)H * W < LD_MAX_PIXELS;
}

extern "C" int as_lidar_zbuf_clear(uint32_t* zbuf, int B, int H, int W, void* stream) {
  AS_CHECK_ARG(zbuf && ld_frame_ok(B, H, W), "as_lidar_zbuf_clear: bad argument (B %d, H %d, W %d)", B, H, W);
  const hipError_t e = hipMemsetAsync(zbuf, 0xFF, (size_t)B * H * W * 4, (hipStream_t)stream);
  if (e != hipSuccess) {
    as_set_error("as_lidar_zbuf_clear: memset failed: %s", hipGetErrorString(e));
    return AS_ERR_LAUNCH;
  }
  return AS_OK;
}

extern "C" int as_lidar_project(const float* points, const int32_t* counts, const double* P, int B, int Nmax, int H, int W,
                                int vel_depth, uint32_t* zbuf, void* stream) {
  AS_CHECK_ARG(points && counts && P && zbuf && ld_frame_ok(B, H, W) && Nmax > 0 && (int64_t)B * Nmax < ((int64_t)1 << 40),
               "as_lidar_project: bad argument (B %d of at most %d, Nmax %d, H %d, W %d)", B, LD_MAX_BATCH, Nmax, H, W);
  AS_CHECK_ARG(((uintptr_t)points & 15) == 0 && ((uintptr_t)P & 7) == 0,
               "as_lidar_project: points must be 16-byte aligned and P 8-byte aligned");
  hipLaunchKernelGGL(lidar_project_kernel, dim3(as_div_up(Nmax, 256), B), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const f32x4*>(points), counts, P, Nmax, H, W, vel_depth, zbuf);
  AS_CHECK_LAUNCH("as_lidar_project");
  return AS_OK;
}

extern "C" int64_t as_lidar_resolve_workspace(int B, int H, int W) {
  if (!ld_frame_ok(B, H, W)) return -1;
  return (int64_t)B * as_div_up((int64_t)H * W, 256) * 6 * 8;
}

extern "C" int as_lidar_resolve(uint32_t* zbuf, int B, int H, int W, int i0, int j0, int h, int w, double bf, int quantize,
                                float* depth_out, float* disp_out, uint16_t* disp_u16, const float* pred, float* metrics,
                                void* workspace, int32_t* overflow, void* stream) {
  AS_CHECK_ARG(zbuf && ld_frame_ok(B, H, W), "as_lidar_resolve: bad argument (B %d of at most %d, H %d, W %d)", B, LD_MAX_BATCH, H, W);
  AS_CHECK_ARG(i0 >= 0 && j0 >= 0 && h > 0 && w > 0 && (int64_t)i0 + h <= H && (int64_t)j0 + w <= W,
               "as_lidar_resolve: window (%d, %d, %d, %d) is not inside %dx%d", i0, j0, h, w, H, W);
  AS_CHECK_ARG(bf > 0.0 && bf < 1e300, "as_lidar_resolve: bf = baseline * fx must be positive and finite (got %g)", bf);
  AS_CHECK_ARG((pred != nullptr) == (metrics != nullptr) && (!pred || (workspace && ((uintptr_t)workspace & 7) == 0)),
               "as_lidar_resolve: pred, metrics and an 8-byte aligned workspace come together");
  hipStream_t st = (hipStream_t)stream;
  if (overflow) {
    const hipError_t e = hipMemsetAsync(overflow, 0, (size_t)B * 4, st);
    if (e != hipSuccess) {
      as_set_error("as_lidar_resolve: memset failed: %s", hipGetErrorString(e));
      return AS_ERR_LAUNCH;
    }
  }
  const int nblk = as_div_up((int64_t)H * W, 256);
  double* partial = static_cast<double*>(workspace);
  hipLaunchKernelGGL(lidar_resolve_kernel, dim3(nblk, B), dim3(256), 0, st, zbuf, H, W, i0, j0, h, w, bf, quantize, depth_out,
                     disp_out, disp_u16, pred, partial, overflow);
  AS_CHECK_LAUNCH("as_lidar_resolve");
  if (pred) {
    hipLaunchKernelGGL(lidar_metrics_kernel, dim3(B), dim3(64), 0, st, partial, nblk, metrics);
    AS_CHECK_LAUNCH("as_lidar_resolve(metrics)");
  }
  return AS_OK;
}
