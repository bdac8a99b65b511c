// Cost-volume probe: per image the two pixels where the feature-contrast map is largest and smallest, their matching curves over
// disparity, and the mean per rank of every pixel's sorted logits: the compute of the reference's
// evaluation/cost_volume_analysis.py:82-92 (feature_contrast_mean, torch.argmax / torch.argmin of the flattened map, the slice,
// torch.sort, sorted[0], sorted[2:].mean(), the ground truth there), in one launch that never leaves the device.
//
// The arithmetic is a CONTRACT (include/adaptive_stereo_hip.h, restated by tests/cv_probe_ref.py):
//   map f      fcs_scores_kernel's mean map (ood.hip): column_stats.h's loop and expression, called here, written out there.
//   selection  torch's argmax / argmin of the flattened map: the first NaN pixel if there is one, else the smallest p holding the
//              extreme.  Every candidate is ONE 64-bit unsigned key, (order(f) << 32) | (0xFFFFFFFF - p): order() maps fp32 values
//              to integers of the same order (-0 and +0 to the same one, NaN to the top; complemented for the minimum), so the
//              unsigned maximum of the keys is the extreme value at the smallest p.  A maximum is associative and commutative: the
//              walk, the butterfly and the merge of the waves cannot disagree, and no lane number enters a comparison.
//   values     the selected pixel's D logits are read again by D lanes (the slice), staged in LDS, and one lane per extreme runs
//              that loop (col_top2_step) over them once more, which also finds d_max: the same code, so the same f.
//   profile    each pixel's D values are sorted in registers by a fixed network (sort_net.h; padding -inf beyond D) and added
//              per rank in fp64: lane t over its pixels in order, xor butterfly over the wave, the waves in order.
//
//   cv_probe_kernel<DMAX, PROFILE>  one workgroup of 512 lanes per image, lane t takes pixels t, t + 512, ...: each of a pixel's D
//              loads is a coalesced row across the wave.  Without the profile the sort and the rank sums are not compiled in.
//              Registers per lane by the compiler's report (no instance uses scratch): 26 / 40 / 60 / 103 without the profile
//              and 38 / 61 / 93 / 217 with it for DMAX 4 / 12 / 24 / 64.  217 fits the 256 a lane has at two waves per SIMD,
//              which is what 512 lanes per workgroup ask for, so the DMAX = 64 instance needs neither fewer lanes nor LDS staging.
//   the cursor launch is cursor.hip's (as_cursor_advance_enqueue).
#include "column_stats.h"
#include "sort_net.h"

#pragma clang fp contract(off)

#define CVP_THREADS 512

// fp32 (not NaN) -> uint32 of the same order, in [0x007FFFFF, 0xFF800000]; -0.f and +0.f give the same integer
__device__ inline uint32_t cvp_order(float f) {
  if (f == 0.f) f = 0.f;
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ inline unsigned long long cvp_max(unsigned long long a, unsigned long long b) { return a > b ? a : b; }

__device__ inline unsigned long long cvp_wave_max(unsigned long long k) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) k = cvp_max(k, __shfl_xor(k, o, 64));
  return k;
}

template <int DMAX, bool PROFILE>
__global__ __launch_bounds__(CVP_THREADS) void cv_probe_kernel(const float* __restrict__ logits, const float* __restrict__ gt, int D,
                                                           int HW, int W, int32_t* __restrict__ pix, float* __restrict__ vals,
                                                           float* __restrict__ slices, float* __restrict__ profile,
                                                           const int32_t* __restrict__ cursor, int capacity) {
  constexpr int NW = CVP_THREADS / 64;
  const int b = blockIdx.x;
  const long row = (long)(cursor ? *cursor : 0) + b;
  if (row < 0 || row >= capacity) return;                  // (uniform) the row has no place: the cursor launch counts it
  const float* vol = logits + (long)b * D * HW;
  const float nan = as_qnan();
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  unsigned long long best_hi = 0, best_lo = 0;              // 0: no pixel yet (every real key is above 2^54)
  double acc[PROFILE ? DMAX : 1];
#pragma unroll
  for (int j = 0; j < (PROFILE ? DMAX : 1); ++j) acc[j] = 0.0;
  bool lane_nan = false;

  for (int p = tid; p < HW; p += CVP_THREADS) {
    const float* l = vol + p;
    float v[DMAX];
    col_load<DMAX>(v, l, D, HW, -INFINITY);                 // the padding sorts behind every real value (descending)
    const ColTop2 st = col_top2<DMAX>(v, D);
    const bool has_nan = st.has_nan;
    const float f = col_fcs(st.m1, st.m2, st.sum, D);
    const uint32_t o = cvp_order(f), low = 0xFFFFFFFFu - (uint32_t)p;
    best_hi = cvp_max(best_hi, ((unsigned long long)(has_nan ? 0xFFFFFFFFu : o) << 32) | low);
    best_lo = cvp_max(best_lo, ((unsigned long long)(has_nan ? 0xFFFFFFFFu : ~o) << 32) | low);

    if (PROFILE) {
      lane_nan = lane_nan || has_nan;
      constexpr SortNet<DMAX> net = make_sort_net<DMAX>();
#pragma unroll
      for (int k = 0; k < net.n; ++k) {
        const float x = v[net.a[k]], y = v[net.b[k]];
        v[net.a[k]] = __builtin_fmaxf(x, y);
        v[net.b[k]] = __builtin_fminf(x, y);
      }
#pragma unroll
      for (int j = 0; j < DMAX; ++j)
        if (j < D) acc[j] += (double)v[j];
    }
  }

  __shared__ unsigned long long keys[2][NW];
  __shared__ float sl[2][AS_COL_MAX_D];
  __shared__ double part[PROFILE ? DMAX : 1][NW];
  best_hi = cvp_wave_max(best_hi);
  best_lo = cvp_wave_max(best_lo);
  if (lane == 0) { keys[0][wave] = best_hi; keys[1][wave] = best_lo; }
  if (PROFILE) {
    const double dnan = __longlong_as_double(0x7FF8000000000000LL);
#pragma unroll
    for (int j = 0; j < DMAX; ++j) {
      if (j < D) {                                           // (uniform)
        const double s = wave_sum_d(lane_nan ? dnan : acc[j]);
        if (lane == 0) part[j][wave] = s;
      }
    }
  }
  __syncthreads();

  if (PROFILE && tid < D) {
    double s = 0.0;
    for (int w = 0; w < NW; ++w) s += part[tid][w];
    profile[row * D + tid] = (float)(s / (double)HW);
  }
  if (!(pix || vals || slices)) return;                    // (uniform)

  // waves 0 and 1: the "hi" and the "lo" pixel
  const int which = wave;                                    // (uniform per wave)
  int p = 0;
  if (which < 2) {
    unsigned long long k = keys[which][0];
    for (int w = 1; w < NW; ++w) k = cvp_max(k, keys[which][w]);
    p = (int)(0xFFFFFFFFu - (uint32_t)k);                    // in [0, HW): HW >= 1, so some lane held a pixel
    if (lane < D) {
      const float x = vol[(long)lane * HW + p];
      sl[which][lane] = x;
      if (slices) slices[(row * 2 + which) * D + lane] = x;
    }
  }
  __syncthreads();
  if (which < 2 && lane == 0) {
    ColTop2 st;
    st.am = -1;                                              // a column of nothing but -inf has no d_max
    for (int d = 0; d < D; ++d) col_top2_step(st, sl[which][d], d);
    float m1 = st.m1, m2 = st.m2, f = col_fcs(m1, m2, st.sum, D);
    float mean_rest = D > 2 ? col_mean_rest(m1, m2, st.sum, D) : nan;
    int d_max = st.am;
    if (st.has_nan) { f = nan; m1 = nan; m2 = nan; mean_rest = nan; d_max = -1; }
    if (pix) {
      int32_t* o = pix + (row * 2 + which) * 3;
      o[0] = p / W; o[1] = p % W; o[2] = d_max;
    }
    if (vals) {
      float* o = vals + (row * 2 + which) * 5;
      o[0] = f; o[1] = m1; o[2] = m2; o[3] = mean_rest;
      o[4] = gt ? gt[(long)b * HW + p] : nan;
    }
  }
}

template <int DMAX>
static void cvp_launch(hipStream_t st, int B, const float* logits, const float* gt, int D, int HW, int W, int32_t* pix, float* vals,
                       float* slices, float* profile, const int32_t* cursor, int capacity) {
  const dim3 grid(B), block(CVP_THREADS);
  if (profile)
    hipLaunchKernelGGL((cv_probe_kernel<DMAX, true>), grid, block, 0, st, logits, gt, D, HW, W, pix, vals, slices, profile, cursor,
                       capacity);
  else
    hipLaunchKernelGGL((cv_probe_kernel<DMAX, false>), grid, block, 0, st, logits, gt, D, HW, W, pix, vals, slices, profile, cursor,
                       capacity);
}

extern "C" int as_cost_volume_probe(const float* logits, const float* gt, int B, int D, int H, int W, int32_t* pix, float* vals,
                                    float* slices, float* profile, int capacity, int32_t* cursor, int32_t* dropped, void* stream) {
  if (int e = as_check_volume("as_cost_volume_probe", logits, B, D, H, W)) return e;
  AS_CHECK_ARG(pix || vals || slices || profile,
               "as_cost_volume_probe: no output requested (pix, vals, slices and profile are all NULL%s)",
               cursor || dropped ? "; cursor and dropped belong to the rows" : "");
  AS_CHECK_ARG(capacity >= 1, "as_cost_volume_probe: capacity %d must be at least 1", capacity);
  hipStream_t st = (hipStream_t)stream;
  const int HW = H * W;
  as_col_dispatch(D, [&](auto dmax) {
    cvp_launch<decltype(dmax)::value>(st, B, logits, gt, D, HW, W, pix, vals, slices, profile, cursor, capacity);
  });
  AS_CHECK_LAUNCH("as_cost_volume_probe");
  if (cursor || dropped) {
    as_cursor_advance_enqueue(st, cursor, dropped, B, capacity);
    AS_CHECK_LAUNCH("as_cost_volume_probe(cursor)");
  }
  return AS_OK;
}
