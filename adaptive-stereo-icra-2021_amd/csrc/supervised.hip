// Supervised two-scale loss (reference train.py:215, utils/loss_functions.py:18-38 with scales = [s, s + k]):
//   total = khamis(pred_disp_l/s, gt) + khamis(pred_disp_l/(s+k), gt),   khamis = sum_{gt>0}(sqrt((gt-p)^2+4)/2 - 1) / max(n, 1)
// Composed from as_khamis_fwd/bwd and as_upsample_bilinear_bwd this is two reductions that each read gt, two element-wise
// derivative maps written to HBM and one of them read back by the up-sampling adjoint.  Here:
//   forward   ONE streaming pass over (gt, refined, up-sampled coarse) + the finalize: both losses, their sum, the count
//   backward  ONE launch: workgroups [0, nadj) are the up-sampling adjoint with the coarse term's derivative formed where the
//             adjoint loads it (never in HBM), the others write the refined map's element-wise derivative
// Per-pixel value and slope: khamis.h, as khamis_fwd_kernel / khamis_bwd_kernel (photometric.hip); sums: fixed-order fp64, two stages.
#include "khamis.h"

#define K2_BLOCKS 512

__global__ __launch_bounds__(256) void khamis2_fwd_kernel(const float* __restrict__ pred0, const float* __restrict__ up,
                                                           const float* __restrict__ gt, long n, double* __restrict__ partial) {
  __shared__ double red[3][4];
  double s0 = 0.0, s1 = 0.0, c = 0.0;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const float g = gt[i];
    if (g > 0.f) {                     // (NaN: not valid)
      s0 += (double)khamis_value(g, pred0[i]);
      s1 += (double)khamis_value(g, up[i]);
      c += 1.0;
    }
  }
  s0 = wave_sum_d(s0); s1 = wave_sum_d(s1); c = wave_sum_d(c);
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = s0; red[1][threadIdx.x >> 6] = s1; red[2][threadIdx.x >> 6] = c; }
  __syncthreads();
  if (threadIdx.x < 3) partial[3 * blockIdx.x + threadIdx.x] =
      red[threadIdx.x][0] + red[threadIdx.x][1] + red[threadIdx.x][2] + red[threadIdx.x][3];
}
__global__ void khamis2_finalize_kernel(const double* __restrict__ partial, int nblk, float* __restrict__ out4) {
  double s0 = 0.0, s1 = 0.0, c = 0.0;
  for (int i = threadIdx.x; i < nblk; i += 64) { s0 += partial[3 * i]; s1 += partial[3 * i + 1]; c += partial[3 * i + 2]; }
  s0 = wave_sum_d(s0); s1 = wave_sum_d(s1); c = wave_sum_d(c);
  if (threadIdx.x == 0) {
    const double nv = c > 1.0 ? c : 1.0;
    const float l0 = (float)(s0 / nv), l1 = (float)(s1 / nv);      // one rounding each: half an ulp of the fp64 quotient
    out4[0] = l0; out4[1] = l1; out4[2] = l0 + l1; out4[3] = (float)nv;
  }
}

// ---- the up-sampling adjoint's coordinates: as resample.hip (bilin_src / footprint / tap_weight), same arithmetic ----------
__device__ inline void k2_bilin_src(float scale, int dst, int in_size, int& i0, int& i1, float& l0, float& l1) {
  float r = scale * ((float)dst + 0.5f) - 0.5f;
  r = r < 0.f ? 0.f : r;
  i0 = (int)r;
  if (i0 > in_size - 1) i0 = in_size - 1;
  i1 = i0 + ((i0 < in_size - 1) ? 1 : 0);
  l1 = r - (float)i0;
  l0 = 1.f - l1;
}
__device__ inline void k2_footprint(float scale, int i, int fine, int& lo, int& hi) {
  lo = (int)floorf(((float)i - 1.f + 0.5f) / scale - 0.5f) - 1;
  hi = (int)ceilf(((float)i + 1.f + 0.5f) / scale - 0.5f) + 1;
  lo = max(lo, 0); hi = min(hi, fine - 1);
}
__device__ inline float k2_tap_weight(float scale, int D, int in_size, int i) {
  int i0, i1; float l0, l1;
  k2_bilin_src(scale, D, in_size, i0, i1, l0, l1);
  return (i0 == i ? l0 : 0.f) + (i1 == i ? l1 : 0.f);
}

#define K2_SPAN 1024
// Workgroups [0, nadj): upsample_bwd_kernel (resample.hip) with its gradient load replaced by the coarse term's derivative at
// that pixel; one workgroup per (image, coarse row, chunk of coarse columns), column sums over the footprint's rows top to
// bottom, then one wave per coarse column.  Workgroups [nadj, gridDim.x): g_pred0, grid-strided.
__global__ __launch_bounds__(256) void khamis2_bwd_kernel(const float* __restrict__ pred0, const float* __restrict__ up,
                                                           const float* __restrict__ gt, const float* __restrict__ g_out3,
                                                           const float* __restrict__ out4, int B, int H, int W, int h, int w,
                                                           float gain, int chunk, int nadj, float* __restrict__ g_pred0,
                                                           float* __restrict__ g_coarse) {
  __shared__ float colsum[K2_SPAN];
  __shared__ float wy_tab[256];
  if ((int)blockIdx.x >= nadj) {
    const float scale = (g_out3[0] + g_out3[2]) / out4[3];
    const long n = (long)B * H * W;
    const long nb = (long)gridDim.x - nadj;
    for (long i = ((long)blockIdx.x - nadj) * 256 + threadIdx.x; i < n; i += nb * 256) {
      const float g = gt[i];
      g_pred0[i] = g > 0.f ? khamis_slope(g, pred0[i], scale) : 0.f;
    }
    return;
  }
  const float scale = (g_out3[1] + g_out3[2]) / out4[3];
  const int nchunks = (w + chunk - 1) / chunk;
  const int c = blockIdx.x % nchunks;
  const int i = (blockIdx.x / nchunks) % h, b = blockIdx.x / (nchunks * h);
  const int j0 = c * chunk, j1 = min(j0 + chunk, w);
  const float sh = (float)h / (float)H, sw = (float)w / (float)W;
  int Y0, Y1, X0, X1, t0, t1;
  k2_footprint(sh, i, H, Y0, Y1);
  k2_footprint(sw, j0, W, X0, t1);
  k2_footprint(sw, j1 - 1, W, t0, X1);
  const float* gq = gt + (long)b * H * W;
  const float* uq = up + (long)b * H * W;
  const int ny = Y1 - Y0 + 1;
  const bool tab = ny <= 256;
  if (tab) wy_tab[threadIdx.x] = (int)threadIdx.x < ny ? k2_tap_weight(sh, Y0 + threadIdx.x, h, i) : 0.f;
  __syncthreads();
  for (int X = X0 + threadIdx.x; X <= X1; X += 256) {
    float acc = 0.f;
    if (tab) {
      for (int Yb = Y0; Yb <= Y1; Yb += 8) {            // eight rows requested together; the sum stays in row order
        float vg[8], vu[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const long at = (long)min(Yb + u, Y1) * W + X;
          vg[u] = gq[at]; vu[u] = uq[at];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u)
          acc += wy_tab[min(Yb + u - Y0, 255)] * (vg[u] > 0.f ? khamis_slope(vg[u], vu[u], scale) : 0.f);
      }
    } else {
      for (int Y = Y0; Y <= Y1; ++Y) {
        const float g = gq[(long)Y * W + X];
        acc += k2_tap_weight(sh, Y, h, i) * (g > 0.f ? khamis_slope(g, uq[(long)Y * W + X], scale) : 0.f);
      }
    }
    colsum[X - X0] = acc;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  for (int j = j0 + (threadIdx.x >> 6); j < j1; j += 4) {
    int a0, a1;
    k2_footprint(sw, j, W, a0, a1);
    float acc = 0.f;
    for (int X = a0 + lane; X <= a1; X += 64) acc += k2_tap_weight(sw, X, w, j) * colsum[X - X0];
    acc = wave_sum(acc);
    if (lane == 0) g_coarse[((long)b * h + i) * w + j] = acc * gain;
  }
}

// ---- host ---------------------------------------------------------------------------------------------------------------
extern "C" int64_t as_khamis2_workspace(int64_t n) { return n > 0 ? 6 * K2_BLOCKS : -1; }

extern "C" int as_khamis2_fwd(const float* pred0, const float* up, const float* gt, int64_t n, float* out4, float* workspace,
                              void* stream) {
  AS_CHECK_ARG(pred0 && up && gt && out4 && workspace && n > 0, "as_khamis2_fwd: bad argument");
  AS_CHECK_ARG(((uintptr_t)workspace & 7) == 0, "as_khamis2_fwd: workspace must be 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  long nb = (n + 255) / 256;
  if (nb > K2_BLOCKS) nb = K2_BLOCKS;
  double* partial = reinterpret_cast<double*>(workspace);
  hipLaunchKernelGGL(khamis2_fwd_kernel, dim3((int)nb), dim3(256), 0, st, pred0, up, gt, (long)n, partial);
  AS_CHECK_LAUNCH("as_khamis2_fwd");
  hipLaunchKernelGGL(khamis2_finalize_kernel, dim3(1), dim3(64), 0, st, partial, (int)nb, out4);
  AS_CHECK_LAUNCH("as_khamis2_fwd(finalize)");
  return AS_OK;
}

extern "C" int as_khamis2_bwd(const float* pred0, const float* up, const float* gt, const float* g_out3, const float* out4,
                              int B, int H, int W, int h, int w, float gain, float* g_pred0, float* g_coarse, void* stream) {
  AS_CHECK_ARG(pred0 && up && gt && g_out3 && out4 && g_pred0 && g_coarse && B > 0 && h > 0 && w > 0 && H > 0 && W > 0,
               "as_khamis2_bwd: bad argument");
  // coarse columns per workgroup: as as_upsample_bilinear_bwd (the chunk's fine footprint within the LDS row of column sums)
  const double inv = (double)W / (double)w;
  int chunk = (int)((252.0 / inv)) - 2;
  if (chunk < 1) chunk = 1;
  if (chunk > w) chunk = w;
  AS_CHECK_ARG((chunk + 2) * inv + 6.0 <= (double)K2_SPAN, "as_khamis2_bwd: scale factor beyond %d fine columns per coarse column", K2_SPAN / 3);
  const long nadj = (long)B * h * ((w + chunk - 1) / chunk);
  const long n = (long)B * H * W;
  long nel = (n + 255) / 256;
  if (nel > 2048) nel = 2048;
  AS_CHECK_ARG(nadj + nel < (1L << 31), "as_khamis2_bwd: too many workgroups");
  hipLaunchKernelGGL(khamis2_bwd_kernel, dim3((unsigned)(nadj + nel)), dim3(256), 0, (hipStream_t)stream, pred0, up, gt, g_out3,
                     out4, B, H, W, h, w, gain, chunk, (int)nadj, g_pred0, g_coarse);
  AS_CHECK_LAUNCH("as_khamis2_bwd");
  return AS_OK;
}
