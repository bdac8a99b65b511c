// Per-image feature-contrast scores (FCS) of a logits volume, for calibrating the OOD gate's threshold: the compute of the
// reference's evaluation/ood_analysis.py:76-77 (feature_contrast_mean(cost_volume).mean(dim=(-2,-1)) per batch, read back per
// batch) and of the other public function of its utils/feature_contrast.py, feature_contrast_median (max - torch.median).
//
// The arithmetic is a CONTRACT (include/adaptive_stereo_hip.h, restated by tests/ood_ref.py):
//   mean map    exactly softargmax_fwd_kernel's fcs (softargmax.hip): the same loop over d in increasing order, the same
//               expression, so the same bits for finite logits.
//   median map  max_d - (element of rank (D-1)/2 in ascending order): two input values and one subtraction.  The element is
//               found by counting, per value, the values that sort in front of it (smaller, or equal with a smaller d); D values
//               stay in registers, D^2 compares, no sort through memory.
//   scores      per image the fp64 sum of each map in a fixed order (per lane over its pixels, butterfly over the wave, waves in
//               order), divided by H*W in fp64, rounded to fp32 once.  No atomics, no workspace: the same input gives the same bits.
//
//   fcs_scores_kernel<DMAX>  one workgroup of 512 lanes per image; lane t takes pixels t, t + 512, ... of the flattened H*W, so
//                            each of a pixel's D loads is a coalesced row across the wave.  It is a latency-bound launch over a few
//                            hundred kilobytes: all D loads of a pixel are issued before the first compare.
//   fcs_advance_kernel       one lane, behind it in stream order: counts the rows that did not fit and advances the cursor.  No
//                            workgroup of the first launch writes what another one of the same launch reads.
#include "as_common.h"

#pragma clang fp contract(off)

#define FCS_MAX_D 64
#define FCS_THREADS 512
#define FCS_MAX_BATCH 65535           // rows of one call; keeps cursor + b inside int32 (the cursor saturates below INT32_MAX - 65535)
#define FCS_CURSOR_MAX (2147483647 - FCS_MAX_BATCH)

template <int DMAX>
__global__ __launch_bounds__(FCS_THREADS) void fcs_scores_kernel(const float* __restrict__ logits, int D, int HW,
                                                                 float* __restrict__ fcs_mean, float* __restrict__ fcs_median,
                                                                 float* __restrict__ scores, const int32_t* __restrict__ cursor,
                                                                 int capacity) {
  const int b = blockIdx.x;
  const float* vol = logits + (long)b * D * HW;
  const bool want_median = fcs_median || scores;        // (uniform)
  const float nan = __int_as_float(0x7FC00000);
  const int rank = (D - 1) / 2;
  double acc_mean = 0.0, acc_med = 0.0;

  for (int pix = threadIdx.x; pix < HW; pix += FCS_THREADS) {
    const float* l = vol + pix;
    float v[DMAX];
#pragma unroll
    for (int d = 0; d < DMAX; ++d) v[d] = d < D ? l[(long)d * HW] : INFINITY;   // the padding sorts behind every real value

    // softargmax_fwd_kernel's loop, over the D real values
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

__global__ void fcs_advance_kernel(int32_t* cursor, int32_t* dropped, int B, int capacity) {
  const int c = cursor ? *cursor : 0;
  if (dropped) {
    long over = (long)c + B - (c > capacity ? c : capacity);      // rows of [c, c + B) at or beyond capacity
    if (c < 0) over = B;                                            // a negative cursor places no row
    if (over > 0) *dropped = (int32_t)(*dropped > 2147483647 - over ? 2147483647 : *dropped + over);
  }
  if (cursor && c >= 0) *cursor = c > FCS_CURSOR_MAX - B ? FCS_CURSOR_MAX : c + B;
}

// the same cursor rule for every collector kernel of the library (entropy.hip appends its rows by it)
void as_cursor_advance_enqueue(hipStream_t st, int32_t* cursor, int32_t* dropped, int B, int capacity) {
  hipLaunchKernelGGL(fcs_advance_kernel, dim3(1), dim3(1), 0, st, cursor, dropped, B, capacity);
}

extern "C" int as_fcs_scores(const float* logits, int B, int D, int H, int W, float* fcs_mean, float* fcs_median, float* scores,
                             int capacity, int32_t* cursor, int32_t* dropped, void* stream) {
  AS_CHECK_ARG(logits && B > 0 && B <= FCS_MAX_BATCH && H > 0 && W > 0 && (int64_t)H * W <= ((int64_t)1 << 30),
               "as_fcs_scores: bad argument (B %d of at most %d, H %d, W %d)", B, FCS_MAX_BATCH, H, W);
  AS_CHECK_ARG(D >= 1 && D <= FCS_MAX_D, "as_fcs_scores: D %d outside [1, %d] (the D values of a pixel are selected in registers)", D,
               FCS_MAX_D);
  AS_CHECK_ARG(fcs_mean || fcs_median || scores, "as_fcs_scores: no output requested");
  AS_CHECK_ARG(scores ? capacity > 0 : (!cursor && !dropped),
               "as_fcs_scores: scores needs capacity > 0 (got %d); cursor and dropped belong to scores", capacity);
  hipStream_t st = (hipStream_t)stream;
  const int HW = H * W;
  const dim3 grid(B), block(FCS_THREADS);
  const int32_t* cur = cursor;
  if (D <= 4)
    hipLaunchKernelGGL(fcs_scores_kernel<4>, grid, block, 0, st, logits, D, HW, fcs_mean, fcs_median, scores, cur, capacity);
  else if (D <= 12)
    hipLaunchKernelGGL(fcs_scores_kernel<12>, grid, block, 0, st, logits, D, HW, fcs_mean, fcs_median, scores, cur, capacity);
  else if (D <= 24)
    hipLaunchKernelGGL(fcs_scores_kernel<24>, grid, block, 0, st, logits, D, HW, fcs_mean, fcs_median, scores, cur, capacity);
  else
    hipLaunchKernelGGL(fcs_scores_kernel<64>, grid, block, 0, st, logits, D, HW, fcs_mean, fcs_median, scores, cur, capacity);
  AS_CHECK_LAUNCH("as_fcs_scores");
  if (cursor || dropped) {
    as_cursor_advance_enqueue(st, cursor, dropped, B, capacity);
    AS_CHECK_LAUNCH("as_fcs_scores(cursor)");
  }
  return AS_OK;
}
