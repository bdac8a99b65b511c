// The post-filter of a full-resolution disparity map before it becomes a point cloud: the discontinuity (flying-pixel) check
// and the speckle filter, the two steps every classical stereo pipeline runs (OpenCV's filterSpeckles, a discontinuity mask) and
// the reference leaves out: its ROS node publishes the raw cloud.  Both are CONTRACTS (include/adaptive_stereo_hip.h, restated
// in numpy by tests/disp_filter_ref.py): integer or selected-float outputs, every fp32 expression a sequence of single IEEE
// operations in the written order, so the results are a pure function of the input whatever order the atomics land in.
//
// All kernels share one geometry: one lane per pixel, lanes along x, a workgroup of DF_SPAN = 256 lanes covers DF_SPAN columns of
// DF_ROWS = 4 consecutive rows, row after row, and strides over the (DF_ROWS x DF_SPAN) tiles of one image; grid (about
// DF_GROUPS / B, B).  A wave is 64 consecutive pixels of one row.
//
//   disp_edge_kernel      a pixel's own disparity and its four neighbours' (the neighbouring lanes' and rows' loads, out of the
//                         cache); max |d - d_q| over the usable neighbours against max(tol_abs, tol_rel * d).  The seven counts
//                         go the way of code_maps.h (as_counts_*).
//
// The speckle filter is connected-component labelling by union-find over the pixel index, label[] being the parent links and
// size[] the root counters (no further workspace).  A parent is never larger than its pixel, a union links the larger root under
// the smaller one, so a root is its component's smallest index: the label the contract asks for.  Four launches, and the hand-off
// between them is the kernel boundary: no lane ever waits for another workgroup, and every loop strictly decreases an index.
//
//   speckle_init_kernel   horizontal runs inside the wave: a ballot of "not joined to the left neighbour" gives every lane the
//                         start of its run in the wave, which becomes its parent (the pixel left of the wave where the run began
//                         before it).  label = parent or -1, size = 0: every call leaves the working state ready for itself.
//   speckle_merge_kernel  vertical unions, only where a run's connection to the row above is NEW: pixel p joins p - W unless its
//                         left neighbour is joined to p, to p - 1 - W and that one to p - W, for then the left neighbour's union (or
//                         one further left) has made the connection already.  Inside this launch a workgroup reads links that
//                         another one is writing, so EVERY access to label[] is an agent-scope atomic: relaxed loads in the find,
//                         atomicMin in the union, which retries from the value the atomic returned when the root it meant to link
//                         was no longer one.  A stale parent is an older, larger link of the same chain: it costs an iteration.
//   speckle_count_kernel  every pixel walks to its root (no union runs any more, so the walk ends at the true root), stores it as
//                         its label (an agent-scope atomic store: other lanes are still walking through it) and counts itself: at
//                         most one integer atomicAdd per distinct root per wave and row, the lanes of a root found by ballot.  The
//                         root that holds most of a row is not added at once: the wave keeps its count over all the rows and tiles
//                         it visits, and the four waves add what they hold through LDS, equal roots together.  One component over
//                         the whole image is then one add per workgroup; added per wave and row, its 7500 adds an image on one
//                         address, which the memory serves one after the other, were most of the pass (measured).
//   speckle_apply_kernel  size = the root's counter (roots keep theirs and are not stored again), the code, valid and counts.
#include "code_maps.h"

#pragma clang fp contract(off)

#define DF_SPAN 256                 // columns a workgroup covers in one row; tests/disp_filter_ref.py places its boundary cases by
#define DF_ROWS 4                   // DF_SPAN, DF_ROWS and DF_WAVE (the 64 pixels of a wave): change them there together with these
#define DF_WAVE 64
#define DF_CODES 7                  // 0 keep, 1-3 as as_lr_check, 4 bad input, 5 discontinuity, 6 speckle
#define DF_GROUPS 2048              // workgroups over all images (8 a CU: every one resident at once)

// (y, x) of every pixel slot of the workgroup's tiles, all 256 lanes of every row together (x may lie beyond W - 1)
template <typename F>
static __device__ inline void df_rows(int H, int xblocks, F f) {
  const long tiles = (long)((H + DF_ROWS - 1) / DF_ROWS) * xblocks;
  for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int ty = (int)(tile / xblocks);
    const int x = (int)(tile - (long)ty * xblocks) * DF_SPAN + threadIdx.x;
    const long y1 = min((long)H, ((long)ty + 1) * DF_ROWS);
    for (int y = ty * DF_ROWS; y < y1; ++y) f(y, x);
  }
}

// usable on top of an incoming code
static __device__ inline bool df_usable(const uint8_t* __restrict__ cin, long at, float d) {
  return (cin == nullptr || cin[at] == 0) && as_disp_usable(d);
}

static inline dim3 df_grid(int B, int H, int W) {
  return as_strided_grid((int64_t)as_div_up(H, DF_ROWS) * as_div_up(W, DF_SPAN), DF_GROUPS, B);
}

// the seven per-lane counts of a workgroup onto counts[b][7]
static __device__ inline void df_add_counts(const int (&mine)[DF_CODES], int* s_count, int32_t* counts) {
#pragma unroll
  for (int c = 0; c < DF_CODES; ++c) as_counts_add(&s_count[c], mine[c]);
  as_counts_flush(s_count, DF_CODES, counts + blockIdx.y * DF_CODES);
}

// ------------------------------------------------------------------------------------------------ the discontinuity check
struct DfEdgeArgs {
  const float* disp;
  const uint8_t* code_in;
  uint8_t* code;
  float* valid;
  float* jump;
  int32_t* counts;
  int H, W, xblocks;
  float tol_abs, tol_rel;
};

__global__ __launch_bounds__(DF_SPAN) void disp_edge_kernel(DfEdgeArgs a) {
  __shared__ int s_count[DF_CODES];
  as_counts_begin(s_count, DF_CODES);
  const int H = a.H, W = a.W;
  const long image = (long)blockIdx.y * H * W;
  const float* D = a.disp + image;
  const uint8_t* K = a.code_in ? a.code_in + image : nullptr;
  int mine[DF_CODES] = {0, 0, 0, 0, 0, 0, 0};
  df_rows(H, a.xblocks, [&](int y, int x) {
    if (x >= W) return;
    const long at = (long)y * W + x;
    const float d = D[at];
    const int cin = K ? K[at] : 0;
    float e = as_qnan();
    int code = cin;
    if (cin == 0) {
      code = 4;
      if (as_disp_usable(d)) {
        const float rel = a.tol_rel * d;
        const float tol = fmaxf(a.tol_abs, rel);
        bool over = false;
        e = 0.f;
        const long q[4] = {at - 1, at + 1, at - W, at + W};
        const bool inside[4] = {x > 0, x < W - 1, y > 0, y < H - 1};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (!inside[k]) continue;
          const float dq = D[q[k]];
          if (!df_usable(K, q[k], dq)) continue;                       // a hole or a rejected pixel is not a jump
          const float eq = fabsf(d - dq);
          e = fmaxf(e, eq);
          over |= eq > tol;
        }
        code = over ? 5 : 0;
      }
    }
    if (a.code) a.code[image + at] = (uint8_t)code;
    if (a.valid) a.valid[image + at] = code == 0 ? 1.f : 0.f;
    if (a.jump) a.jump[image + at] = e;
#pragma unroll
    for (int c = 0; c < DF_CODES; ++c) mine[c] += code == c;
  });
  if (a.counts == nullptr) return;                                     // uniform: no lane waits below
  df_add_counts(mine, s_count, a.counts);
}

extern "C" int as_disp_edge_check(const float* disp, const uint8_t* code_in, int B, int H, int W, float tol_abs, float tol_rel,
                                  uint8_t* code, float* valid, float* jump, int32_t* counts, void* stream) {
  AS_CHECK_ARG(disp, "as_disp_edge_check: null pointer");
  if (int rc = as_check_images("as_disp_edge_check", B, H, W, true)) return rc;
  AS_CHECK_ARG(tol_abs >= 0.f && tol_rel >= 0.f, "as_disp_edge_check: tol_abs %g and tol_rel %g must be numbers and not negative",
               tol_abs, tol_rel);
  AS_CHECK_ARG(code || valid || jump || counts, "as_disp_edge_check: no output requested");
  AS_CHECK_ARG(!counts || ((uintptr_t)counts & 3) == 0, "as_disp_edge_check: counts must be 4-byte aligned");
  const int64_t n = (int64_t)B * H * W;
  const AsRange r[] = {{disp, n * 4}, {code_in, n}, {code, n}, {valid, n * 4}, {jump, n * 4}, {counts, (int64_t)B * DF_CODES * 4}};
  AS_CHECK_ARG(as_disjoint(r, 2, 6), "as_disp_edge_check: an output may alias neither an input nor another output (overlapping ranges)");
  hipStream_t st = (hipStream_t)stream;
  if (int rc = as_clear_counts("as_disp_edge_check", counts, B * DF_CODES, st)) return rc;
  DfEdgeArgs a;
  a.disp = disp; a.code_in = code_in; a.code = code; a.valid = valid; a.jump = jump; a.counts = counts;
  a.H = H; a.W = W; a.xblocks = as_div_up(W, DF_SPAN);
  a.tol_abs = tol_abs; a.tol_rel = tol_rel;
  hipLaunchKernelGGL(disp_edge_kernel, df_grid(B, H, W), dim3(DF_SPAN), 0, st, a);
  AS_CHECK_LAUNCH("as_disp_edge_check");
  return AS_OK;
}

// ------------------------------------------------------------------------------------------------ the speckle filter
struct DfSpeckleArgs {
  const float* disp;
  const uint8_t* code_in;
  int32_t* label;
  int32_t* size;
  uint8_t* code;
  float* valid;
  int32_t* counts;
  int H, W, xblocks, max_size;
  float max_diff;
};

#define DF_LOAD(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)

// the root of p as far as this lane can see it: parents are never larger than the pixel, so p strictly decreases
static __device__ inline int spk_find(int32_t* L, int p) {
  int q;
  while ((q = DF_LOAD(L + p)) < p && q >= 0) p = q;
  return p;
}

// joins the sets of a and b: the larger root goes under the smaller one.  When the atomic shows that `a` was no root any more
// (it returns a's parent of that moment, below a), that parent takes a's place: max(a, b) strictly decreases.
static __device__ inline void spk_union(int32_t* L, int a, int b) {
  for (;;) {
    a = spk_find(L, a);
    b = spk_find(L, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(L + a, b);
    if (old == a) return;
    a = old;
  }
}

__global__ __launch_bounds__(DF_SPAN) void speckle_init_kernel(DfSpeckleArgs a) {
  const int W = a.W;
  const long image = (long)blockIdx.y * a.H * W;
  const float* D = a.disp + image;
  const uint8_t* K = a.code_in ? a.code_in + image : nullptr;
  const int lane = threadIdx.x & 63;
  df_rows(a.H, a.xblocks, [&](int y, int x) {
    const bool in = x < W;
    const long at = (long)y * W + x;
    const float d = in ? D[at] : 0.f;
    const int us = in && df_usable(K, at, d);
    float dl = __shfl_up(d, 1, 64);
    int usl = __shfl_up(us, 1, 64);
    if (lane == 0) {
      usl = 0;
      if (in && x > 0) {
        dl = D[at - 1];
        usl = df_usable(K, at - 1, dl);
      }
    }
    const bool joined = us && usl && fabsf(d - dl) <= a.max_diff;
    const unsigned long long starts = __ballot(!joined);                // lanes that begin a run (or hold no pixel)
    if (!in) return;
    const unsigned long long upto = starts & (~0ull >> (63 - lane));
    // the run began in this wave at the highest start at or below the lane, or before the wave: then the pixel left of the wave
    const int back = upto ? lane - (63 - __clzll((long long)upto)) : lane + 1;
    a.label[image + at] = us ? (int)at - back : -1;
    a.size[image + at] = 0;
  });
}

__global__ __launch_bounds__(DF_SPAN) void speckle_merge_kernel(DfSpeckleArgs a) {
  const int W = a.W;
  const long image = (long)blockIdx.y * a.H * W;
  const float* D = a.disp + image;
  const uint8_t* K = a.code_in ? a.code_in + image : nullptr;
  int32_t* L = a.label + image;
  const int lane = threadIdx.x & 63;
  const float md = a.max_diff;
  df_rows(a.H, a.xblocks, [&](int y, int x) {
    if (y == 0) return;                                                // uniform over the workgroup
    const bool in = x < W;
    const long at = (long)y * W + x;
    const float d = in ? D[at] : 0.f, du = in ? D[at - W] : 0.f;
    const int us = in && df_usable(K, at, d), usu = in && df_usable(K, at - W, du);
    const int jup = us && usu && fabsf(d - du) <= md;
    float dl = __shfl_up(d, 1, 64), dul = __shfl_up(du, 1, 64);
    int usl = __shfl_up(us, 1, 64), usul = __shfl_up(usu, 1, 64), jupl = __shfl_up(jup, 1, 64);
    if (lane == 0) {
      usl = usul = jupl = 0;
      if (in && x > 0) {
        dl = D[at - 1]; dul = D[at - W - 1];
        usl = df_usable(K, at - 1, dl); usul = df_usable(K, at - W - 1, dul);
        jupl = usl && usul && fabsf(dl - dul) <= md;
      }
    }
    // the left neighbour's column is joined vertically and to this one in both rows: the connection is not new
    const bool covered = jupl && usl && fabsf(d - dl) <= md && usul && fabsf(du - dul) <= md;
    if (jup && !covered) spk_union(L, (int)at, (int)(at - W));
  });
}

__global__ __launch_bounds__(DF_SPAN) void speckle_count_kernel(DfSpeckleArgs a) {
  const int W = a.W;
  const long image = (long)blockIdx.y * a.H * W;
  int32_t* L = a.label + image;
  int32_t* S = a.size + image;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int held_root = -1, held = 0;                                        // uniform over the wave: pixels of one root not yet added
  df_rows(a.H, a.xblocks, [&](int y, int x) {
    int root = -1;
    if (x < W) {
      const int p = (int)((long)y * W + x);
      const int parent = DF_LOAD(L + p);
      if (parent >= 0) {
        root = spk_find(L, parent);
        if (root != parent) __hip_atomic_store(L + p, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    unsigned long long todo = __ballot(root >= 0);                     // uniform over the wave; loses a bit or more a turn
    while (todo) {
      const int lead = __ffsll((long long)todo) - 1;
      const int r = __shfl(root, lead, 64);
      const unsigned long long same = __ballot(root == r) & todo;
      const int n = __popcll(same);
      if (r == held_root) {
        held += n;
      } else if (held == 0 || n > DF_WAVE / 2) {                       // the root of most of this row takes the held place
        if (held && lane == 0) atomicAdd(S + held_root, held);
        held_root = r;
        held = n;
      } else if (lane == lead) {
        atomicAdd(S + r, n);
      }
      todo &= ~same;
    }
  });
  // what the four waves still hold: equal roots together, one add each
  __shared__ int s_root[DF_SPAN / DF_WAVE], s_held[DF_SPAN / DF_WAVE];
  if (lane == 0) { s_root[wave] = held_root; s_held[wave] = held; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 0; w < DF_SPAN / DF_WAVE; ++w) {
      int n = s_held[w];
      if (n == 0) continue;
      for (int v = w + 1; v < DF_SPAN / DF_WAVE; ++v)
        if (s_held[v] && s_root[v] == s_root[w]) { n += s_held[v]; s_held[v] = 0; }
      atomicAdd(S + s_root[w], n);
    }
  }
}

__global__ __launch_bounds__(DF_SPAN) void speckle_apply_kernel(DfSpeckleArgs a) {
  __shared__ int s_count[DF_CODES];
  as_counts_begin(s_count, DF_CODES);
  const int W = a.W;
  const long image = (long)blockIdx.y * a.H * W;
  const uint8_t* K = a.code_in ? a.code_in + image : nullptr;
  const int32_t* L = a.label + image;
  int32_t* S = a.size + image;
  int mine[DF_CODES] = {0, 0, 0, 0, 0, 0, 0};
  df_rows(a.H, a.xblocks, [&](int y, int x) {
    if (x >= W) return;
    const long at = (long)y * W + x;
    const int root = L[at];
    const int cin = K ? K[at] : 0;
    int sz = 0;
    if (root >= 0) {
      sz = S[root];                                                    // a root's counter: no lane of this launch stores there
      if (root != (int)at) S[at] = sz;
    }
    const int code = cin != 0 ? cin : root < 0 ? 4 : sz <= a.max_size ? 6 : 0;
    if (a.code) a.code[image + at] = (uint8_t)code;
    if (a.valid) a.valid[image + at] = code == 0 ? 1.f : 0.f;
#pragma unroll
    for (int c = 0; c < DF_CODES; ++c) mine[c] += code == c;
  });
  if (a.counts == nullptr) return;                                     // uniform: no lane waits below
  df_add_counts(mine, s_count, a.counts);
}

extern "C" int as_disp_speckle(const float* disp, const uint8_t* code_in, int B, int H, int W, float max_diff, int max_size,
                               int32_t* label, int32_t* size, uint8_t* code, float* valid, int32_t* counts, void* stream) {
  AS_CHECK_ARG(disp && label && size, "as_disp_speckle: null pointer");
  if (int rc = as_check_images("as_disp_speckle", B, H, W, true)) return rc;
  AS_CHECK_ARG(max_diff >= 0.f, "as_disp_speckle: max_diff %g must be a number and not negative", max_diff);
  AS_CHECK_ARG(max_size >= 0, "as_disp_speckle: max_size %d must not be negative", max_size);
  AS_CHECK_ARG((((uintptr_t)label | (uintptr_t)size | (uintptr_t)counts) & 3) == 0,
               "as_disp_speckle: label, size and counts must be 4-byte aligned");
  const int64_t n = (int64_t)B * H * W;
  const AsRange r[] = {{disp, n * 4}, {code_in, n}, {label, n * 4}, {size, n * 4}, {code, n}, {valid, n * 4},
                       {counts, (int64_t)B * DF_CODES * 4}};
  AS_CHECK_ARG(as_disjoint(r, 2, 7), "as_disp_speckle: an output may alias neither an input nor another output (overlapping ranges)");
  hipStream_t st = (hipStream_t)stream;
  if (int rc = as_clear_counts("as_disp_speckle", counts, B * DF_CODES, st)) return rc;
  DfSpeckleArgs a;
  a.disp = disp; a.code_in = code_in; a.label = label; a.size = size; a.code = code; a.valid = valid; a.counts = counts;
  a.H = H; a.W = W; a.xblocks = as_div_up(W, DF_SPAN); a.max_size = max_size;
  a.max_diff = max_diff;
  const dim3 grid = df_grid(B, H, W);
  hipLaunchKernelGGL(speckle_init_kernel, grid, dim3(DF_SPAN), 0, st, a);
  if (H > 1) hipLaunchKernelGGL(speckle_merge_kernel, grid, dim3(DF_SPAN), 0, st, a);
  hipLaunchKernelGGL(speckle_count_kernel, grid, dim3(DF_SPAN), 0, st, a);
  hipLaunchKernelGGL(speckle_apply_kernel, grid, dim3(DF_SPAN), 0, st, a);
  AS_CHECK_LAUNCH("as_disp_speckle");
  return AS_OK;
}
