// What the stages around the network's disparity share (lr_consistency.hip, disp_filter.hip, sgm.hip): they write a per-pixel code
// map and count the pixels of each code.  One definition each of "a disparity is usable", of the counters' way from a lane to
// global memory, of their clear, and of the shape refusals and the grid of a launch that strides over the images of a batch.
#pragma once
#include "as_common.h"

// as_lr_check's step 1: a number, not negative, not +inf.  -0.0 is usable.
static __device__ __forceinline__ bool as_disp_usable(float d) { return d >= 0.f && d != INFINITY; }

// ---- per-code counters of a workgroup --------------------------------------------------------------------------------------
// A lane counts in registers; as_counts_add sums one such count over the wave and adds it to one LDS integer; as_counts_flush
// ends as one global integer atomic per non-zero slot and workgroup, onto counters the entry point has cleared: exact in any
// order.  The counters of a batch share a cache line or two, where atomics serialise, hence the detour through LDS.
//   __shared__ int s_count[N];  as_counts_begin(s_count, N);  ... the tile loop ...
//   if (counts == nullptr) return;        // uniform over the launch: no lane may reach flush's barrier when others skip it
//   as_counts_add(&s_count[c], mine[c]) for every slot that is fed;  as_counts_flush(s_count, N, counts + <this workgroup's N>);
static __device__ __forceinline__ void as_counts_begin(int* s_count, int n) {
  if (threadIdx.x < (unsigned)n) s_count[threadIdx.x] = 0;
  __syncthreads();
}
static __device__ __forceinline__ void as_counts_add(int* s_slot, int mine) {
  const int v = wave_sum_i(mine);
  if ((threadIdx.x & 63) == 0 && v) atomicAdd(s_slot, v);
}
static __device__ __forceinline__ void as_counts_flush(const int* s_count, int n, int32_t* dst) {
  __syncthreads();
  if (threadIdx.x < (unsigned)n && s_count[threadIdx.x]) atomicAdd(dst + threadIdx.x, s_count[threadIdx.x]);
}

// counts[0 .. n) = 0 before the launch that adds to them; NULL: nothing to do.  A kernel launch (as_zero_i32_enqueue) and not
// hipMemsetAsync: a memset node of a captured graph was seen to fill with a stale pattern from its second replay on (cursor.hip).
static inline int as_clear_counts(const char* who, int32_t* counts, int n, hipStream_t st) {
  if (counts == nullptr) return AS_OK;
  as_zero_i32_enqueue(st, counts, n);
  AS_CHECK_LAUNCH(who);
  return AS_OK;
}

// ---- a batch of B images of H x W pixels, image b on blockIdx.y --------------------------------------------------------------
// pixel_index: the kernels index an image's pixels (or count them) in int32
static inline int as_check_images(const char* who, int B, int H, int W, bool pixel_index) {
  AS_CHECK_ARG(B > 0 && H > 0 && W > 0, "%s: bad shape (B %d, H %d, W %d)", who, B, H, W);
  AS_CHECK_ARG(!pixel_index || (int64_t)H * W <= 0x7FFFFFFF, "%s: H * W = %lld overflows an int32 pixel index", who, (long long)H * W);
  AS_CHECK_ARG(B <= 65535, "%s: B %d above 65535, the grid's second extent", who, B);
  return AS_OK;
}

// The grid of a launch whose workgroups stride over the `tiles` of one image (and view): about `groups` workgroups over all
// images and views, never more than an image has tiles.
static inline dim3 as_strided_grid(int64_t tiles, int groups, int B, int views = 1) {
  const int64_t per_image = as_div_up(groups, (int64_t)views * B);
  return dim3((unsigned)(tiles < per_image ? tiles : per_image), B, views);
}
