// Per-pixel confidence of the coarse disparity from the logits volume, and the binned error statistics that calibrate a gate on
// it.  The reference has no counterpart: it uses the post-aggregation matching distribution only through the image mean of its
// feature-contrast score.  The maps are the standard confidence measures of the stereo literature taken on the soft-max of the
// aggregated volume: the probability of the mode, one minus the normalised entropy, and the probability mass within
// one coarse disparity of the mode, which is what exposes a bimodal column (the soft-argmax, a mean, lies on neither surface).
//
// The arithmetic is a CONTRACT (include/adaptive_stereo_hip.h, restated in fp64 by tests/confidence_ref.py): every fp32 expression
// is a sequence of single IEEE operations in the written order, so nothing here may contract into an fma.
//
//   disp_confidence_kernel<DMAX>  one lane per coarse pixel, lanes along W, grid ceil(H*W/256) x B: each of a pixel's D loads is a
//                                 coalesced row across the wave.  The load and the arg-max pass are column_stats.h's (col_load,
//                                 col_top2; DMAX = 4 / 12 / 24 / 64).  No atomics, no workspace, no LDS.  It is a latency-bound
//                                 launch over a few hundred kilobytes and needs no tuning beyond that.
//   sparsification_kernel         grid-stride over the n elements; every workgroup keeps count / bad / abs_err of the K bins in LDS
//                                 (integer and fp64 LDS atomics), then adds its non-empty bins to the global arrays: one 64-bit
//                                 integer add each for count and bad, one fp64 add for abs_err.  The integers are exact in any
//                                 order; the fp64 sum is order-dependent in its last bits (bound: n 2^-53 times the bin's sum).
#include "column_stats.h"

#pragma clang fp contract(off)

#define SP_MAX_K 1024
#define SP_THREADS 256
#define SP_MAX_BLOCKS 512
#define SP_MAX_N ((int64_t)1 << 40)   // a workgroup's share stays below 2^31: its LDS counters are 32 bit

typedef unsigned long long u64;

template <int DMAX>
__global__ __launch_bounds__(256) void disp_confidence_kernel(const float* __restrict__ logits, int D, int HW, float* __restrict__ pmax,
                                                              float* __restrict__ cent, float* __restrict__ mass) {
  const int b = blockIdx.y;
  const int pix = blockIdx.x * 256 + threadIdx.x;
  if (pix >= HW) return;
  const float* l = logits + (long)b * D * HW + pix;
  float v[DMAX];
  col_load<DMAX>(v, l, D, HW, -INFINITY);
  const ColTop2 st = col_top2<DMAX>(v, D);                // the mode and where it is first reached
  const float m1 = st.m1;
  const int a = st.am;
  // a NaN, a +inf (without a NaN it is the maximum) or nothing but -inf
  const bool bad = st.has_nan || m1 == INFINITY || m1 == -INFINITY;

  float se = 0.f, T = 0.f, e_lo = 0.f, e_at = 0.f, e_hi = 0.f;
#pragma unroll
  for (int d = 0; d < DMAX; ++d) {
    if (d < D) {
      const float t = v[d] - m1;
      const float e = expf(t);
      se += e;
      const float et = e * t;
      T += e == 0.f ? 0.f : et;
      e_lo = d == a - 1 ? e : e_lo;
      e_at = d == a ? e : e_at;
      e_hi = d == a + 1 ? e : e_hi;
    }
  }
  float p = 1.f / se;
  float ms = ((e_lo + e_at) + e_hi) / se;
  const float Hn = logf(se) - T / se;
  float c = 1.f - Hn / logf((float)D);
  c = fminf(fmaxf(c, 0.f), 1.f);
  if (D == 1) { p = 1.f; ms = 1.f; c = 1.f; }
  if (bad) p = ms = c = as_qnan();

  const long at = (long)b * HW + pix;
  if (pmax) pmax[at] = p;
  if (cent) cent[at] = c;
  if (mass) mass[at] = ms;
}

__global__ __launch_bounds__(SP_THREADS) void sparsification_kernel(const float* __restrict__ key, const float* __restrict__ pred,
                                                                     const float* __restrict__ gt, long n, float lo, float scale, int K,
                                                                     float tau, u64* __restrict__ count, u64* __restrict__ bad,
                                                                     double* __restrict__ abs_err, u64* __restrict__ skipped) {
  __shared__ uint32_t s_count[SP_MAX_K];
  __shared__ uint32_t s_bad[SP_MAX_K];
  __shared__ double s_err[SP_MAX_K];
  __shared__ uint32_t s_skipped;
  for (int k = threadIdx.x; k < K; k += SP_THREADS) {
    s_count[k] = 0;
    s_bad[k] = 0;
    s_err[k] = 0.0;
  }
  if (threadIdx.x == 0) s_skipped = 0;
  __syncthreads();

  const long stride = (long)gridDim.x * SP_THREADS;
  for (long i = (long)blockIdx.x * SP_THREADS + threadIdx.x; i < n; i += stride) {
    const float g = gt[i];
    if (!(g > 0.f)) continue;                             // as eval_metrics_kernel: strict >, drops NaN
    const float kv = key[i];
    const float err = fabsf(pred[i] - g);
    if (kv != kv || err != err) {
      atomicAdd(&s_skipped, 1u);
      continue;
    }
    const float t = (kv - lo) * scale;
    const int k = t < 0.f ? 0 : (t >= (float)K ? K - 1 : (int)t);
    atomicAdd(&s_count[k], 1u);
    if (err > tau) atomicAdd(&s_bad[k], 1u);
    atomicAdd(&s_err[k], (double)err);
  }
  __syncthreads();

  for (int k = threadIdx.x; k < K; k += SP_THREADS) {
    const uint32_t c = s_count[k];
    if (c) {
      atomicAdd(count + k, (u64)c);
      if (s_bad[k]) atomicAdd(bad + k, (u64)s_bad[k]);
      atomicAdd(abs_err + k, s_err[k]);
    }
  }
  if (threadIdx.x == 0 && s_skipped) atomicAdd(skipped, (u64)s_skipped);
}

extern "C" int as_disp_confidence(const float* logits, int B, int D, int H, int W, float* pmax, float* cent, float* mass,
                                  void* stream) {
  if (int e = as_check_volume("as_disp_confidence", logits, B, D, H, W)) return e;
  AS_CHECK_ARG(pmax || cent || mass, "as_disp_confidence: no output requested");
  hipStream_t st = (hipStream_t)stream;
  const int HW = H * W;
  as_col_dispatch(D, [&](auto dmax) {
    hipLaunchKernelGGL(disp_confidence_kernel<decltype(dmax)::value>, dim3(as_div_up(HW, 256), B), dim3(256), 0, st, logits, D, HW,
                       pmax, cent, mass);
  });
  AS_CHECK_LAUNCH("as_disp_confidence");
  return AS_OK;
}

extern "C" int as_sparsification(const float* key, const float* pred, const float* gt, int64_t n, float lo, float scale, int K,
                                 float tau, int64_t* count, int64_t* bad, double* abs_err, int64_t* skipped, void* stream) {
  AS_CHECK_ARG(key && pred && gt && count && bad && abs_err && skipped, "as_sparsification: null pointer");
  AS_CHECK_ARG(n > 0 && n <= SP_MAX_N && K >= 1 && K <= SP_MAX_K, "as_sparsification: bad argument (n %lld in [1, 2^40], K %d in [1, %d])",
               (long long)n, K, SP_MAX_K);
  AS_CHECK_ARG(lo - lo == 0.f && scale > 0.f && scale - scale == 0.f && tau == tau,
               "as_sparsification: lo %g must be finite, scale %g positive and finite, tau %g not NaN", lo, scale, tau);
  AS_CHECK_ARG((((uintptr_t)count | (uintptr_t)bad | (uintptr_t)abs_err | (uintptr_t)skipped) & 7) == 0,
               "as_sparsification: the outputs must be 8-byte aligned");
  int64_t nb = (n + SP_THREADS * 8 - 1) / (SP_THREADS * 8);
  if (nb > SP_MAX_BLOCKS) nb = SP_MAX_BLOCKS;
  hipLaunchKernelGGL(sparsification_kernel, dim3((int)nb), dim3(SP_THREADS), 0, (hipStream_t)stream, key, pred, gt, (long)n, lo, scale,
                     K, tau, reinterpret_cast<u64*>(count), reinterpret_cast<u64*>(bad), abs_err, reinterpret_cast<u64*>(skipped));
  AS_CHECK_LAUNCH("as_sparsification");
  return AS_OK;
}
