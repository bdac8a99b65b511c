// The proxy-label term of the adaptation loss: the Khamis loss of the network's disparity against the semi-global matcher's,
// over the pixels every stage of sgm.ProxyLabeler kept, read where the labeler leaves them (the matcher's disp_l, the speckle
// pass's final code).  Composed from what exists this is torch.eq + torch.where over the map (labels = code == 0 ? disp : 0),
// then as_khamis_fwd, and it says nothing about how far the network is from the matcher.  Here:
//   forward   ONE streaming pass over (pred, disp, code) + the one-wave finalize: the loss, its sum and count, the mean
//             |disp - pred| and the share of labelled pixels beyond bad_px
//   backward  ONE element-wise launch
// A pixel carries a label iff code == 0 && disp > 0.f (NaN, -0.0, 0.0, negatives, every non-zero code: none), which is the set
// where(code == 0, disp, 0) > 0 that as_khamis_fwd sees on the materialised labels.
// Forward access widths: loss, sum and count are bit for bit as_khamis_fwd's, so element i belongs to lane i % 256 of workgroup
// (i / 256) % gridDim.x and every lane adds its elements in rising order; a lane therefore loads 4 bytes of pred and disp and 1
// of code per element (a wave reads 256 contiguous bytes per map), four trips of the stride loop in flight, at any alignment.
// The backward has no order to keep: 16 bytes per lane and map where the three fp32 bases allow it, code as one word or four
// bytes, a scalar tail for n % 4; every base off 16 bytes takes the scalar loop for all of it.
#include "as_common.h"
#include <math.h>
// no contraction from here on, as in photometric.hip: khamis_slope then rounds d * d and + 4 separately, which is what makes
// as_proxy_term_bwd bit for bit as_khamis_bwd
#pragma clang fp contract(off)
#include "khamis.h"

__device__ inline bool proxy_labelled(unsigned code, float disp) { return code == 0u && disp > 0.f; }

__global__ __launch_bounds__(256) void proxy_term_fwd_kernel(const float* __restrict__ pred, const float* __restrict__ disp,
                                                              const uint8_t* __restrict__ code, long n, float bad_px,
                                                              double* __restrict__ partial) {
  __shared__ double red[4][4];
  double s = 0.0, c = 0.0, e = 0.0, b = 0.0;
  const long stride = (long)gridDim.x * 256;
  for (long i0 = (long)blockIdx.x * 256 + threadIdx.x; i0 < n; i0 += 4 * stride) {
    float g[4], p[4];
    unsigned k[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {                     // the loads of four trips, requested together
      const long i = i0 + u * stride;
      const bool in = i < n;
      g[u] = in ? disp[i] : 0.f;
      p[u] = in ? pred[i] : 0.f;
      k[u] = in ? (unsigned)code[i] : 1u;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {                     // consumed in trip order: the lane's sums keep as_khamis_fwd's order
      if (proxy_labelled(k[u], g[u])) {
        const float err = fabsf(g[u] - p[u]);
        s += (double)khamis_value(g[u], p[u]); c += 1.0;
        e += (double)err; b += err > bad_px ? 1.0 : 0.0;
      }
    }
  }
  s = wave_sum_d(s); c = wave_sum_d(c); e = wave_sum_d(e); b = wave_sum_d(b);
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = s; red[1][threadIdx.x >> 6] = c; red[2][threadIdx.x >> 6] = e; red[3][threadIdx.x >> 6] = b;
  }
  __syncthreads();
  if (threadIdx.x < 4) partial[4 * blockIdx.x + threadIdx.x] =
      red[threadIdx.x][0] + red[threadIdx.x][1] + red[threadIdx.x][2] + red[threadIdx.x][3];
}
__global__ void proxy_term_finalize_kernel(const double* __restrict__ partial, int nblk, float* __restrict__ out6) {
  double s = 0.0, c = 0.0, e = 0.0, b = 0.0;
  for (int i = threadIdx.x; i < nblk; i += 64) {
    s += partial[4 * i]; c += partial[4 * i + 1]; e += partial[4 * i + 2]; b += partial[4 * i + 3];
  }
  s = wave_sum_d(s); c = wave_sum_d(c); e = wave_sum_d(e); b = wave_sum_d(b);
  if (threadIdx.x == 0) {
    const double nv = c > 1.0 ? c : 1.0;
    out6[0] = (float)s / (float)nv;          // as khamis_finalize_kernel: the fp32 sum by the count, in fp32
    out6[1] = (float)nv;
    out6[2] = (float)s;
    out6[3] = (float)(e / nv);               // one rounding of the fp64 quotient each
    out6[4] = (float)(b / nv);
    out6[5] = (float)c;
  }
}

// g_pred = *g_loss / out6[1] * d value / d pred on the labelled pixels, 0.f elsewhere.  vec: the three fp32 bases are 16-byte
// aligned; code_word: code is 4-byte aligned.
__global__ __launch_bounds__(256) void proxy_term_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ disp,
                                                              const uint8_t* __restrict__ code, const float* __restrict__ g_loss,
                                                              const float* __restrict__ out6, long n, int vec, int code_word,
                                                              float* __restrict__ g_pred) {
  const float scale = g_loss[0] / out6[1];
  const long stride = (long)gridDim.x * 256, t = (long)blockIdx.x * 256 + threadIdx.x;
  long done = 0;
  if (vec) {
    const long n4 = n >> 2;
    for (long q = t; q < n4; q += stride) {
      const f32x4 g = reinterpret_cast<const f32x4*>(disp)[q], p = reinterpret_cast<const f32x4*>(pred)[q];
      unsigned k;
      if (code_word) {
        k = reinterpret_cast<const uint32_t*>(code)[q];
      } else {
        const uint8_t* kq = code + 4 * q;
        k = (unsigned)kq[0] | (unsigned)kq[1] << 8 | (unsigned)kq[2] << 16 | (unsigned)kq[3] << 24;
      }
      f32x4 r;
#pragma unroll
      for (int u = 0; u < 4; ++u) r[u] = proxy_labelled((k >> (8 * u)) & 255u, g[u]) ? khamis_slope(g[u], p[u], scale) : 0.f;
      reinterpret_cast<f32x4*>(g_pred)[q] = r;
    }
    done = n4 << 2;
  }
  for (long i = done + t; i < n; i += stride) {
    const float g = disp[i];
    g_pred[i] = proxy_labelled(code[i], g) ? khamis_slope(g, pred[i], scale) : 0.f;
  }
}

// ---- host ---------------------------------------------------------------------------------------------------------------
extern "C" int64_t as_proxy_term_workspace(int64_t n) { return n > 0 ? 8 * MS_BLOCKS : -1; }

extern "C" int as_proxy_term_fwd(const float* pred, const float* disp, const uint8_t* code, int64_t n, float bad_px, float* out6,
                                 float* workspace, void* stream) {
  AS_CHECK_ARG(pred && disp && code && out6 && workspace, "as_proxy_term_fwd: null pointer");
  AS_CHECK_ARG(n > 0, "as_proxy_term_fwd: n %lld must be positive", (long long)n);
  AS_CHECK_ARG(((uintptr_t)workspace & 7) == 0, "as_proxy_term_fwd: workspace must be 8-byte aligned");
  AS_CHECK_ARG((((uintptr_t)pred | (uintptr_t)disp | (uintptr_t)out6) & 3) == 0, "as_proxy_term_fwd: pred, disp and out6 must be 4-byte aligned");
  AS_CHECK_ARG(bad_px >= 0.f && !isinf(bad_px), "as_proxy_term_fwd: bad_px %g must be finite and not negative", (double)bad_px);
  const AsRange r[5] = {{pred, 4 * n}, {disp, 4 * n}, {code, n}, {out6, 24}, {workspace, 4 * as_proxy_term_workspace(n)}};
  AS_CHECK_ARG(as_disjoint(r, 3, 5), "as_proxy_term_fwd: out6 and workspace must not alias an input or each other");
  hipStream_t st = (hipStream_t)stream;
  long nb = (n + 255) / 256;
  if (nb > MS_BLOCKS) nb = MS_BLOCKS;
  double* partial = reinterpret_cast<double*>(workspace);
  hipLaunchKernelGGL(proxy_term_fwd_kernel, dim3((int)nb), dim3(256), 0, st, pred, disp, code, (long)n, bad_px, partial);
  AS_CHECK_LAUNCH("as_proxy_term_fwd");
  hipLaunchKernelGGL(proxy_term_finalize_kernel, dim3(1), dim3(64), 0, st, partial, (int)nb, out6);
  AS_CHECK_LAUNCH("as_proxy_term_fwd(finalize)");
  return AS_OK;
}

extern "C" int as_proxy_term_bwd(const float* pred, const float* disp, const uint8_t* code, const float* g_loss, const float* out6,
                                 int64_t n, float* g_pred, void* stream) {
  AS_CHECK_ARG(pred && disp && code && g_loss && out6 && g_pred, "as_proxy_term_bwd: null pointer");
  AS_CHECK_ARG(n > 0, "as_proxy_term_bwd: n %lld must be positive", (long long)n);
  AS_CHECK_ARG((((uintptr_t)pred | (uintptr_t)disp | (uintptr_t)g_loss | (uintptr_t)out6 | (uintptr_t)g_pred) & 3) == 0,
               "as_proxy_term_bwd: the fp32 arguments must be 4-byte aligned");
  const AsRange r[6] = {{pred, 4 * n}, {disp, 4 * n}, {code, n}, {g_loss, 4}, {out6, 24}, {g_pred, 4 * n}};
  AS_CHECK_ARG(as_disjoint(r, 5, 6), "as_proxy_term_bwd: g_pred must not alias an input");
  const int vec = (((uintptr_t)pred | (uintptr_t)disp | (uintptr_t)g_pred) & 15) == 0 && n >= 4;
  const int code_word = ((uintptr_t)code & 3) == 0;
  const long work = vec ? (n + 3) / 4 : n;
  long nb = (work + 255) / 256;
  if (nb > 2048) nb = 2048;
  hipLaunchKernelGGL(proxy_term_bwd_kernel, dim3((int)nb), dim3(256), 0, (hipStream_t)stream, pred, disp, code, g_loss, out6, (long)n,
                     vec, code_word, g_pred);
  AS_CHECK_LAUNCH("as_proxy_term_bwd");
  return AS_OK;
}
