// Per-image feature-contrast scores (FCS) of a logits volume, for calibrating the OOD gate's threshold: the compute of the
// reference's evaluation/ood_analysis.py:76-77 (feature_contrast_mean(cost_volume).mean(dim=(-2,-1)) per batch, read back per
// batch) and of the other public function of its utils/feature_contrast.py, feature_contrast_median (max - torch.median).
//
// The arithmetic is a CONTRACT (include/adaptive_stereo_hip.h, restated by tests/ood_ref.py):
//   mean map    the loop and expression defined in column_stats.h, which softargmax_fwd_kernel (softargmax.hip) and
//               cv_probe_kernel call.  Here they are WRITTEN OUT, statement for statement: every form that called the header
//               (the whole loop, the step alone, the expression alone) gave this kernel another schedule that measured
//               0.6 - 1.3 % slower at D = 24 (profiles/column_stats_timing.txt).  tests/test_gpu_cv_probe.py
//               (test_the_three_fcs_maps_are_one_map) and tests/test_gpu_ood.py hold the copy to the callers bit for bit.
//   median map  max_d - (element of rank (D-1)/2 in ascending order): two input values and one subtraction.  The element is
//               found by counting, per value, the values that sort in front of it (smaller, or equal with a smaller d); D values
//               stay in registers, D^2 compares, no sort through memory.
//   scores      per image the fp64 sum of each map in a fixed order (per lane over its pixels, butterfly over the wave, waves in
//               order), divided by H*W in fp64, rounded to fp32 once.  No atomics, no workspace: the same input gives the same bits.
//
//   fcs_scores_kernel<DMAX>  one workgroup of 512 lanes per image; lane t takes pixels t, t + 512, ... of the flattened H*W, so
//                            each of a pixel's D loads is a coalesced row across the wave.  It is a latency-bound launch over a few
//                            hundred kilobytes: all D loads of a pixel are issued before the first compare.
//   the cursor launch behind it is cursor.hip's (as_cursor_advance_enqueue).
#include "column_stats.h"

#pragma clang fp contract(off)

#define FCS_THREADS 512

template <int DMAX>
__global__ __launch_bounds__(FCS_THREADS) void fcs_scores_kernel(const float* __restrict__ logits, int D, int HW,
                                                                 float* __restrict__ fcs_mean, float* __restrict__ fcs_median,
                                                                 float* __restrict__ scores, const int32_t* __restrict__ cursor,
                                                                 int capacity) {
  const int b = blockIdx.x;
  const float* vol = logits + (long)b * D * HW;
  const bool want_median = fcs_median || scores;        // (uniform)
  const float nan = as_qnan();
  const int rank = (D - 1) / 2;
  double acc_mean = 0.0, acc_med = 0.0;

  for (int pix = threadIdx.x; pix < HW; pix += FCS_THREADS) {
    const float* l = vol + pix;
    float v[DMAX];
#pragma unroll
    for (int d = 0; d < DMAX; ++d) v[d] = d < D ? l[(long)d * HW] : INFINITY;   // the padding sorts behind every real value

    // column_stats.h's col_load, col_top2 and col_fcs, written out (see the note above)
    float m1 = -INFINITY, m2 = -INFINITY, sum = 0.f;
    bool has_nan = false;
#pragma unroll
    for (int d = 0; d < DMAX; ++d) {
      if (d < D) {
        const float x = v[d];
        sum += x;
        if (x > m1) { m2 = m1; m1 = x; }
        else if (x > m2) { m2 = x; }
        has_nan = has_nan || x != x;
      }
    }
    float mean = (D > 2) ? m1 - (sum - m1 - m2) / (float)(D - 2) : 0.f;
    if (has_nan) mean = nan;

    float med = 0.f;
    if (want_median) {
      float sel = v[0];
#pragma unroll
      for (int i = 0; i < DMAX; ++i) {
        int before = 0;
#pragma unroll
        for (int j = 0; j < DMAX; ++j) before += (v[j] < v[i] || (j < i && v[j] == v[i])) ? 1 : 0;
        if (before == rank) sel = v[i];                  // exactly one i among the real values when none is NaN
      }
      med = has_nan ? nan : m1 - sel;
    }

    if (fcs_mean) fcs_mean[(long)b * HW + pix] = mean;
    if (fcs_median) fcs_median[(long)b * HW + pix] = med;
    acc_mean += (double)mean;
    acc_med += (double)med;
  }
  if (!scores) return;                                    // (uniform)

  __shared__ double part[2][FCS_THREADS / 64];
  acc_mean = wave_sum_d(acc_mean);
  acc_med = wave_sum_d(acc_med);
  if ((threadIdx.x & 63) == 0) {
    part[0][threadIdx.x >> 6] = acc_mean;
    part[1][threadIdx.x >> 6] = acc_med;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    double s = 0.0;
    for (int w = 0; w < FCS_THREADS / 64; ++w) s += part[threadIdx.x][w];
    const long row = (long)(cursor ? *cursor : 0) + b;
    if (row >= 0 && row < capacity) scores[2 * row + threadIdx.x] = (float)(s / (double)HW);
  }
}

extern "C" int as_fcs_scores(const float* logits, int B, int D, int H, int W, float* fcs_mean, float* fcs_median, float* scores,
                             int capacity, int32_t* cursor, int32_t* dropped, void* stream) {
  if (int e = as_check_volume("as_fcs_scores", logits, B, D, H, W)) return e;
  AS_CHECK_ARG(fcs_mean || fcs_median || scores, "as_fcs_scores: no output requested");
  AS_CHECK_ARG(scores ? capacity > 0 : (!cursor && !dropped),
               "as_fcs_scores: scores needs capacity > 0 (got %d); cursor and dropped belong to scores", capacity);
  hipStream_t st = (hipStream_t)stream;
  const int HW = H * W;
  as_col_dispatch(D, [&](auto dmax) {
    hipLaunchKernelGGL(fcs_scores_kernel<decltype(dmax)::value>, dim3(B), dim3(FCS_THREADS), 0, st, logits, D, HW, fcs_mean,
                       fcs_median, scores, (const int32_t*)cursor, capacity);
  });
  AS_CHECK_LAUNCH("as_fcs_scores");
  if (cursor || dropped) {
    as_cursor_advance_enqueue(st, cursor, dropped, B, capacity);
    AS_CHECK_LAUNCH("as_fcs_scores(cursor)");
  }
  return AS_OK;
}
