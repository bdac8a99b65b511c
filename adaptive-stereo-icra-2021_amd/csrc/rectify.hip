// Stereo rectification of raw camera pairs on the device: the stage between "the camera delivers bytes" and the network's input.
// The reference has none (ros/stereo_depth_node.py feeds imgmsg_to_cv2(...)/255 to the network, which is right only behind a
// rectifying driver); a host pipeline runs cv2.initUndistortRectifyMap once and cv2.remap per frame.
//
// The arithmetic is a CONTRACT (include/adaptive_stereo_hip.h, restated op for op by tests/rectify_ref.py): every fp32 expression
// is a sequence of single IEEE operations in the written order, so nothing here may contract into an fma, and every division is
// the correctly rounded one.
//
//   rc_coord            the ONE coordinate function: rectified pixel -> ray -> distorted raw pixel and its validity.  Both kernels
//                       call it, so what as_rectify_map reports is what as_rectify_pair sampled.
//   rectify_map_kernel  one lane per pixel; called once when a rectifier is built.
//   rectify_pair_kernel both cameras and the whole batch in one launch (the image is the grid's z: [0, B) left, [B, 2B) right).
//                       A workgroup is 4 rows x 64 lanes and covers RC_ROWS rows x RC_SPAN columns, RC_PX pixels per lane.  The
//                       coordinates are recomputed per frame and not read from a stored map: 3 B read + 12 B written per pixel
//                       as it is, a map would add 8 B.  A lane owns pixels lane, lane + 64, lane + 128, lane + 192 of the span:
//                       the byte gathers of a wave then fall into a few cache lines and its dword stores are 256 contiguous
//                       bytes, each guarded against the row's end.  The other shape (a lane owns 4 CONSECUTIVE pixels and writes
//                       16 bytes per plane where W % 4 == 0) was built and measured: 34.5 us against 25.5 us at 4 x 375 x 1242,
//                       because the gathers, not the stores, bound the kernel and that shape spreads each of them over four
//                       times the addresses.  It is not kept: one route.
#include "as_common.h"

#pragma clang fp contract(off)

#define RC_PX 4                       // pixels per lane
#define RC_LANES 64                   // lanes along x: one wave per row of the tile
#define RC_ROWS 4                     // rows per workgroup
#define RC_SPAN (RC_PX * RC_LANES)    // columns per workgroup
#define RC_MAX_IMAGES 65535           // 2 * B: images are the grid's z dimension
#define RC_MAX_OFFSET (1 << 30)       // |i0|, |j0|: x + j0 stays inside int32

struct RcCoord {
  float us, vs;
  bool valid;
};

struct RcFrame {
  int H0, W0, i0, j0, H, W;
};

__device__ inline RcCoord rc_coord(const as_rectify_camera& c, const RcFrame& f, int x, int y) {
  const float u = (float)(x + f.j0), v = (float)(y + f.i0);
  const float X = (c.m[0] * u + c.m[1] * v) + c.m[2];
  const float Y = (c.m[3] * u + c.m[4] * v) + c.m[5];
  const float Z = (c.m[6] * u + c.m[7] * v) + c.m[8];
  const float xn = X / Z, yn = Y / Z;
  const float xx = xn * xn, yy = yn * yn, xy = xn * yn, r2 = xx + yy;
  const float num = ((c.k3 * r2 + c.k2) * r2 + c.k1) * r2 + 1.f;
  const float den = ((c.k6 * r2 + c.k5) * r2 + c.k4) * r2 + 1.f;
  const float rad = num / den;
  const float xd = (xn * rad + (2.f * c.p1) * xy) + c.p2 * (r2 + 2.f * xx);
  const float yd = (yn * rad + c.p1 * (r2 + 2.f * yy)) + (2.f * c.p2) * xy;
  RcCoord r;
  r.us = c.fx * xd + c.cx;
  r.vs = c.fy * yd + c.cy;
  r.valid = Z > 0.f && r.us >= 0.f && r.us <= (float)(f.W0 - 1) && r.vs >= 0.f && r.vs <= (float)(f.H0 - 1);   // a NaN fails
  return r;
}

__global__ __launch_bounds__(256) void rectify_map_kernel(as_rectify_camera cam, RcFrame f, float* __restrict__ map_x,
                                                          float* __restrict__ map_y, float* __restrict__ valid) {
  const long o = (long)blockIdx.x * 256 + threadIdx.x;
  if (o >= (long)f.H * f.W) return;
  const int y = (int)(o / f.W), x = (int)(o - (long)y * f.W);
  const RcCoord r = rc_coord(cam, f, x, y);
  if (map_x) map_x[o] = r.us;
  if (map_y) map_y[o] = r.vs;
  if (valid) valid[o] = r.valid ? 1.f : 0.f;
}

// the four taps of one channel around a VALID coordinate: top = (b-a)*ax + a; bot = (d-c)*ax + c; (bot-top)*ay + top; / 255
__device__ inline float rc_sample(const uint8_t* __restrict__ r0, const uint8_t* __restrict__ r1, int o0, int o1, float ax, float ay) {
  const float a = (float)r0[o0], b = (float)r0[o1], c = (float)r1[o0], d = (float)r1[o1];
  const float top = (b - a) * ax + a;
  const float bot = (d - c) * ax + c;
  const float val = (bot - top) * ay + top;
  return val / 255.f;
}

template <int C>
__global__ __launch_bounds__(RC_LANES * RC_ROWS) void rectify_pair_kernel(const uint8_t* __restrict__ src_l,
                                                                          const uint8_t* __restrict__ src_r, int B,
                                                                          as_rectify_camera cam_l, as_rectify_camera cam_r, RcFrame f,
                                                                          float fill, float* __restrict__ dst_l,
                                                                          float* __restrict__ dst_r) {
  const int y = blockIdx.y * RC_ROWS + threadIdx.y;
  if (y >= f.H) return;
  const bool right = (int)blockIdx.z >= B;                      // (uniform)
  const int b = right ? (int)blockIdx.z - B : (int)blockIdx.z;
  const as_rectify_camera& cam = right ? cam_r : cam_l;
  const uint8_t* __restrict__ src = (right ? src_r : src_l) + (long)b * f.H0 * f.W0 * C;
  const long plane = (long)f.H * f.W;
  float* __restrict__ dst = (right ? dst_r : dst_l) + (long)b * 3 * plane + (long)y * f.W;
  const int xb = blockIdx.x * RC_SPAN;

  float out[3][RC_PX];
#pragma unroll
  for (int k = 0; k < RC_PX; ++k) {
    const int x = xb + threadIdx.x + k * RC_LANES;
    out[0][k] = out[1][k] = out[2][k] = fill;
    if (x >= f.W) continue;
    const RcCoord r = rc_coord(cam, f, x, y);
    if (!r.valid) continue;
    // only now: the coordinates of an invalid pixel may be NaN, infinite or beyond int32
    const float fx0 = floorf(r.us), fy0 = floorf(r.vs);
    const int x0 = (int)fx0, y0 = (int)fy0;
    const int x1 = min(x0 + 1, f.W0 - 1), y1 = min(y0 + 1, f.H0 - 1);
    const float ax = r.us - (float)x0, ay = r.vs - (float)y0;
    const uint8_t* __restrict__ r0 = src + (long)y0 * f.W0 * C;
    const uint8_t* __restrict__ r1 = src + (long)y1 * f.W0 * C;
    if (C == 1) {
      out[0][k] = out[1][k] = out[2][k] = rc_sample(r0, r1, x0, x1, ax, ay);
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c) out[c][k] = rc_sample(r0, r1, x0 * 3 + c, x1 * 3 + c, ax, ay);
    }
  }

#pragma unroll
  for (int k = 0; k < RC_PX; ++k) {
    const int x = xb + threadIdx.x + k * RC_LANES;
    if (x < f.W) {
#pragma unroll
      for (int c = 0; c < 3; ++c) dst[c * plane + x] = out[c][k];
    }
  }
}

static bool rc_frame_ok(int H0, int W0, int i0, int j0, int H, int W) {
  return H0 > 0 && W0 > 0 && H > 0 && W > 0 && i0 >= -RC_MAX_OFFSET && i0 <= RC_MAX_OFFSET && j0 >= -RC_MAX_OFFSET &&
         j0 <= RC_MAX_OFFSET && (int64_t)H * W < ((int64_t)1 << 30) && (int64_t)H0 * W0 < ((int64_t)1 << 30);
}

extern "C" int as_rectify_map(const as_rectify_camera* cam, int H0, int W0, int i0, int j0, int H, int W, float* map_x, float* map_y,
                              float* valid, void* stream) {
  AS_CHECK_ARG(cam && rc_frame_ok(H0, W0, i0, j0, H, W),
               "as_rectify_map: bad argument (raw %dx%d, window %dx%d at (%d, %d); offsets within +-2^30, fewer than 2^30 pixels)", H0,
               W0, H, W, i0, j0);
  AS_CHECK_ARG(map_x || map_y || valid, "as_rectify_map: no output requested");
  const RcFrame f = {H0, W0, i0, j0, H, W};
  hipLaunchKernelGGL(rectify_map_kernel, dim3(as_div_up((int64_t)H * W, 256)), dim3(256), 0, (hipStream_t)stream, *cam, f, map_x,
                     map_y, valid);
  AS_CHECK_LAUNCH("as_rectify_map");
  return AS_OK;
}

extern "C" int as_rectify_pair(const uint8_t* src_l, const uint8_t* src_r, int B, int H0, int W0, int C, const as_rectify_camera* cam_l,
                               const as_rectify_camera* cam_r, int i0, int j0, int H, int W, float fill, float* dst_l, float* dst_r,
                               void* stream) {
  AS_CHECK_ARG(src_l && src_r && cam_l && cam_r && dst_l && dst_r, "as_rectify_pair: a NULL pointer");
  AS_CHECK_ARG(B > 0 && 2 * (int64_t)B <= RC_MAX_IMAGES && (C == 1 || C == 3), "as_rectify_pair: bad argument (B %d of at most %d, C %d: 1 or 3)",
               B, RC_MAX_IMAGES / 2, C);
  AS_CHECK_ARG(rc_frame_ok(H0, W0, i0, j0, H, W),
               "as_rectify_pair: bad argument (raw %dx%d, window %dx%d at (%d, %d); offsets within +-2^30, fewer than 2^30 pixels)", H0,
               W0, H, W, i0, j0);
  AS_CHECK_ARG(((uintptr_t)dst_l & 3) == 0 && ((uintptr_t)dst_r & 3) == 0, "as_rectify_pair: the outputs must be 4-byte aligned");
  AS_CHECK_ARG(as_div_up(H, RC_ROWS) <= 65535, "as_rectify_pair: H %d needs more than 65535 row tiles", H);
  const RcFrame f = {H0, W0, i0, j0, H, W};
  const dim3 grid(as_div_up(W, RC_SPAN), as_div_up(H, RC_ROWS), 2 * B), block(RC_LANES, RC_ROWS);
  hipStream_t st = (hipStream_t)stream;
  if (C == 1)
    hipLaunchKernelGGL(rectify_pair_kernel<1>, grid, block, 0, st, src_l, src_r, B, *cam_l, *cam_r, f, fill, dst_l, dst_r);
  else
    hipLaunchKernelGGL(rectify_pair_kernel<3>, grid, block, 0, st, src_l, src_r, B, *cam_l, *cam_r, f, fill, dst_l, dst_r);
  AS_CHECK_LAUNCH("as_rectify_pair");
  return AS_OK;
}
