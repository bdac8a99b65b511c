// The row cursor of the collector kernels (as_fcs_scores, as_image_entropy, as_cost_volume_probe): a launch writes its B rows at
// *cursor + b where they fit, and this one-lane launch behind it in stream order counts the rows that did not and advances the
// cursor.  No workgroup of the first launch writes what another one of the same launch reads.
#include "as_common.h"

#define CURSOR_MAX (2147483647 - AS_CURSOR_MAX_BATCH)     // the cursor saturates here, so cursor + b never leaves int32

__global__ void cursor_advance_kernel(int32_t* cursor, int32_t* dropped, int B, int capacity) {
  const int c = cursor ? *cursor : 0;
  if (dropped) {
    long over = (long)c + B - (c > capacity ? c : capacity);      // rows of [c, c + B) at or beyond capacity
    if (c < 0) over = B;                                            // a negative cursor places no row
    if (over > 0) *dropped = (int32_t)(*dropped > 2147483647 - over ? 2147483647 : *dropped + over);
  }
  if (cursor && c >= 0) *cursor = c > CURSOR_MAX - B ? CURSOR_MAX : c + B;
}

void as_cursor_advance_enqueue(hipStream_t st, int32_t* cursor, int32_t* dropped, int B, int capacity) {
  hipLaunchKernelGGL(cursor_advance_kernel, dim3(1), dim3(1), 0, st, cursor, dropped, B, capacity);
}

// Counters cleared by a KERNEL node, not by hipMemsetAsync: a memset node of a captured graph was seen (ROCm 7.2, MI355X) to fill
// with a stale 16-byte pattern from its second replay on (the counters then came out as that pattern plus the counts), the first
// replay and every eager call being right.  A kernel's arguments are part of its node.
__global__ void zero_i32_kernel(int32_t* p, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) p[i] = 0;
}

void as_zero_i32_enqueue(hipStream_t st, int32_t* p, int n) {
  hipLaunchKernelGGL(zero_i32_kernel, dim3(as_div_up(n, 256)), dim3(256), 0, st, p, n);
}
