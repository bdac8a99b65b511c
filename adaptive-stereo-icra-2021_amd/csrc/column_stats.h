// The statistics of ONE COLUMN of a logits volume [B][D][H][W] (the D values of a pixel), defined once: the top-2 / sum loop and
// the feature-contrast expression of the contract in include/adaptive_stereo_hip.h, the "all D loads first, D values in
// registers" load, and the host side every column kernel shares (the DMAX ladder, the limits, the argument check).
//
// Callers: softargmax_fwd_kernel (softargmax.hip), cv_probe_kernel (cv_probe.hip, its walk and its lane-0 pass over the selected
// slice) and disp_confidence_kernel (confidence.hip).  They give the same bits for the same column because they run this code,
// in increasing d.  Two kernels keep a written-out copy, each with a comment that names this file:
//   fcs_scores_kernel (ood.hip)   every form that called into this header gave it another schedule, 0.6 - 1.3 % slower at
//                                 D = 24 (profiles/column_stats_timing.txt); the GPU tests hold its map to the callers' bit for bit.
//   the fused tail (agg_tail.hip) splits a column over eight lanes and merges the partial states, so it adds in another order
//                                 and differs in the last bits.  It calls col_fcs; its per-lane step is col_top2_step written
//                                 out, because the call changed that file's register allocation, and the tail is on the timed path.
//
// No expression here has a multiply feeding an add or a subtract, so there is nothing for the compiler to contract into an fma:
// the header gives the same bits whatever fp-contract setting the includer has.
//
// The scalar part compiles as plain C++ (tests/tools/column_stats_check.cpp runs it on the host).
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#include <type_traits>

#include "as_common.h"
#define AS_COL_FN __host__ __device__ inline
#else
#define AS_COL_FN inline
#endif

// m1 >= m2 the two largest values so far (m2 == m1 when the maximum occurs twice), sum the fp32 sum in the order of the steps,
// am the index of the FIRST maximum (left as it starts while no value is above -inf).  NaN compares false: it enters sum only.
struct ColTop2 {
  float m1 = -INFINITY, m2 = -INFINITY, sum = 0.f;
  int am = 0;
  bool has_nan = false;
};

AS_COL_FN void col_top2_step(ColTop2& st, float x, int d) {
  st.sum += x;
  if (x > st.m1) { st.m2 = st.m1; st.m1 = x; st.am = d; }
  else if (x > st.m2) { st.m2 = x; }
  st.has_nan = st.has_nan || x != x;
}

// the mean of the D - 2 values below the top two; D > 2
AS_COL_FN float col_mean_rest(float m1, float m2, float sum, int D) { return (sum - m1 - m2) / (float)(D - 2); }

// the feature-contrast score: max minus the mean of the rest, 0 for D <= 2
AS_COL_FN float col_fcs(float m1, float m2, float sum, int D) { return (D > 2) ? m1 - col_mean_rest(m1, m2, sum, D) : 0.f; }

// v[d] = the column's value at d (l + d * HW) for d < D, `pad` beyond: fully unrolled, so all D loads are issued before the first
// use and v stays in registers.  -inf pads for a maximum or a descending sort, +inf where the padding must sort behind.
template <int DMAX>
AS_COL_FN void col_load(float (&v)[DMAX], const float* l, int D, long HW, float pad) {
#pragma unroll
  for (int d = 0; d < DMAX; ++d) v[d] = d < D ? l[(long)d * HW] : pad;
}

// the loop over the D real values of a loaded column
template <int DMAX>
AS_COL_FN ColTop2 col_top2(const float (&v)[DMAX], int D) {
  ColTop2 st;
#pragma unroll
  for (int d = 0; d < DMAX; ++d)
    if (d < D) col_top2_step(st, v[d], d);
  return st;
}

#if defined(__HIPCC__)
// ---- host side of a column kernel ------------------------------------------------------------------------------------------
#define AS_COL_MAX_D 64                          // the widest instance: 64 values per lane still fit the registers
#define AS_COL_MAX_BATCH AS_CURSOR_MAX_BATCH     // images are a grid dimension, and rows of one collector call

// f(std::integral_constant<int, DMAX>) with the narrowest built DMAX >= D; 1 <= D <= AS_COL_MAX_D
template <class F>
static inline void as_col_dispatch(int D, F&& f) {
  if (D <= 4) f(std::integral_constant<int, 4>());
  else if (D <= 12) f(std::integral_constant<int, 12>());
  else if (D <= 24) f(std::integral_constant<int, 24>());
  else f(std::integral_constant<int, 64>());
}

static inline int as_check_volume(const char* who, const float* logits, int B, int D, int H, int W) {
  AS_CHECK_ARG(logits && B > 0 && B <= AS_COL_MAX_BATCH && H > 0 && W > 0 && (int64_t)H * W <= ((int64_t)1 << 30),
               "%s: bad argument (B %d of at most %d, H %d, W %d)", who, B, AS_COL_MAX_BATCH, H, W);
  AS_CHECK_ARG(D >= 1 && D <= AS_COL_MAX_D, "%s: D %d outside [1, %d] (the D values of a pixel stay in registers)", who, D,
               AS_COL_MAX_D);
  return AS_OK;
}
#endif
