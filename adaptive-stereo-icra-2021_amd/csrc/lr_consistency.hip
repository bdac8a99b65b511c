// Both-view inference around the network: the mirrored input batches, the flip back, the left-right consistency check of the two
// disparity maps and the background fill of what the check rejects.  The reference holds only the first half
// (predict_disparity_leftright, adapt.py:40-62: two torch.cat of a torch.flip, and a torch.flip per output); the check and the
// fill are the classical post-processing of the stereo literature and have no counterpart there.
//
// The arithmetic of the check is a CONTRACT (include/adaptive_stereo_hip.h, restated in numpy by tests/lr_consistency_ref.py):
// every fp32 expression is a sequence of single IEEE operations in the written order, so nothing here may contract into an fma.
// Mirror, flip and fill only move or select values and are bit-exact by construction.
//
//   mirror_pair_kernel<V>    one lane per V = 4, 2 or 1 floats of the two inputs, a workgroup inside one row; each is read once
//                            and stored twice, once as it is and once mirrored in x into the other batch.  V needs W % V == 0
//                            and bases aligned to 4 V bytes.
//   flip_w_kernel<V>         the same for one map.
//   lr_check_kernel          one lane per pixel and view, lanes along x; a workgroup strides over the (row, 256 columns) tiles of
//                            one image and view, grid (about 2048 / 2B, B, 2): a coalesced load of the pixel's own disparity and
//                            a gather of two neighbours out of the other view's row, which the neighbouring workgroups stream
//                            through the cache.  The five counts go the way of code_maps.h (as_counts_*).  The counters of a batch
//                            share one or two cache lines, where atomics serialise, so the workgroups are kept to about 2048
//                            instead of one per tile.
//   lr_fill_kernel           one workgroup of 256 lanes per row, FILL_ITEMS pixels per lane, so a pass covers FILL_SPAN = 1024
//                            pixels.  "The last code-0 value so far" is an associative operator (the right operand wins when it
//                            holds a value): FILL_ITEMS serial steps in registers, an inclusive scan over the wave with
//                            __shfl_up, the four wave totals through LDS, and a carry from pass to pass in a register.  The
//                            forward scan leaves every pixel's left neighbour in `out`; the backward scan is the same code over
//                            the mirrored index and picks the smaller of the two.  Whether a pixel has a left neighbour at all
//                            is "it lies right of the row's first code-0 pixel", which the forward scan reduces on the way.
#include "code_maps.h"

#pragma clang fp contract(off)

#define LR_THREADS 256
#define LR_CODES 5
#define LR_CHECK_GROUPS 2048        // workgroups of the check over all images and views (8 a CU: every one resident at once)
#define LR_MAX_W (1 << 24)          // (float)x is exact below 2^24
#define FILL_ITEMS 4                // tests/lr_consistency_ref.py places its boundary cases by FILL_SPAN (1024) and FILL_WAVE (256 =
                                    // 64 * FILL_ITEMS): change them there, and the 1024 in the header, together with this
#define FILL_SPAN (LR_THREADS * FILL_ITEMS)

// ------------------------------------------------------------------------------------------------ mirror, flip
typedef float f32x2 __attribute__((ext_vector_type(2)));
template <int V> struct LrVec;
template <> struct LrVec<1> { typedef float T; static __device__ inline T reversed(T v) { return v; } };
template <> struct LrVec<2> { typedef f32x2 T; static __device__ inline T reversed(T v) { return T{v.y, v.x}; } };
template <> struct LrVec<4> { typedef f32x4 T; static __device__ inline T reversed(T v) { return T{v.w, v.z, v.y, v.x}; } };

// V floats a lane; a workgroup takes 256 groups of V out of ONE row (Wq groups a row, xchunks workgroups a row), so the row is one
// 32-bit division per workgroup and not a 64-bit one per lane.  half: floats of one input
template <int V>
__global__ __launch_bounds__(LR_THREADS) void mirror_pair_kernel(const float* __restrict__ left, const float* __restrict__ right,
                                                                 int Wq, int xchunks, long half, float* __restrict__ left_batch,
                                                                 float* __restrict__ right_batch) {
  typedef typename LrVec<V>::T T;
  const unsigned row = blockIdx.x / (unsigned)xchunks;
  const int x = (int)(blockIdx.x - row * (unsigned)xchunks) * LR_THREADS + threadIdx.x;
  if (x >= Wq) return;
  const long i = (long)row * Wq + x, m = (long)row * Wq + (Wq - 1 - x);      // the group and its mirror image in the row
  const T l = reinterpret_cast<const T*>(left)[i], r = reinterpret_cast<const T*>(right)[i];
  reinterpret_cast<T*>(left_batch)[i] = l;
  reinterpret_cast<T*>(right_batch)[i] = r;
  reinterpret_cast<T*>(left_batch + half)[m] = LrVec<V>::reversed(r);
  reinterpret_cast<T*>(right_batch + half)[m] = LrVec<V>::reversed(l);
}

template <int V>
__global__ __launch_bounds__(LR_THREADS) void flip_w_kernel(const float* __restrict__ src, int Wq, int xchunks, float* __restrict__ dst) {
  typedef typename LrVec<V>::T T;
  const unsigned row = blockIdx.x / (unsigned)xchunks;
  const int x = (int)(blockIdx.x - row * (unsigned)xchunks) * LR_THREADS + threadIdx.x;
  if (x >= Wq) return;
  reinterpret_cast<T*>(dst)[(long)row * Wq + (Wq - 1 - x)] = LrVec<V>::reversed(reinterpret_cast<const T*>(src)[(long)row * Wq + x]);
}

// floats a lane moves at once: 4 or 2 when they divide W (then every row starts as aligned as the base) and every base is aligned
static inline int lr_vector_width(int W, const void* a, const void* b, const void* c = nullptr, const void* d = nullptr) {
  const uintptr_t bits = (uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d;
  if (W % 4 == 0 && (bits & 15) == 0) return 4;
  if (W % 2 == 0 && (bits & 7) == 0) return 2;
  return 1;
}

// `rows` rows of W floats as these kernels cover them: ceil(W / 256) workgroups a row at one float a lane (the most), all in a 1-D
// grid.  The product is taken in double, where int32 factors cannot overflow; what passes is exact in int64.
static inline bool lr_rows_ok(double rows, int W) { return rows * as_div_up(W, LR_THREADS) <= 2147483647.0; }

template <int V>
static void mirror_pair_launch(hipStream_t st, const float* left, const float* right, int64_t rows, int W, float* left_batch,
                               float* right_batch) {
  const int Wq = W / V, xchunks = as_div_up(Wq, LR_THREADS);
  hipLaunchKernelGGL(mirror_pair_kernel<V>, dim3((unsigned)(rows * xchunks)), dim3(LR_THREADS), 0, st, left, right, Wq, xchunks,
                     (long)(rows * W), left_batch, right_batch);
}

extern "C" int as_mirror_pair(const float* left, const float* right, int B, int C, int H, int W, float* left_batch, float* right_batch,
                              void* stream) {
  AS_CHECK_ARG(left && right && left_batch && right_batch, "as_mirror_pair: null pointer");
  AS_CHECK_ARG(B > 0 && C > 0 && H > 0 && W > 0, "as_mirror_pair: bad shape (B %d, C %d, H %d, W %d)", B, C, H, W);
  AS_CHECK_ARG(lr_rows_ok((double)B * C * H, W), "as_mirror_pair: %.0f rows of %d elements exceed the grid", (double)B * C * H, W);
  const int64_t rows = (int64_t)B * C * H;
  const int64_t in_bytes = rows * W * 4, out_bytes = 2 * in_bytes;
  const AsRange r[] = {{left, in_bytes}, {right, in_bytes}, {left_batch, out_bytes}, {right_batch, out_bytes}};
  AS_CHECK_ARG(as_disjoint(r, 2, 4), "as_mirror_pair: the outputs may alias neither each other nor an input (overlapping ranges)");
  hipStream_t st = (hipStream_t)stream;
  switch (lr_vector_width(W, left, right, left_batch, right_batch)) {
    case 4: mirror_pair_launch<4>(st, left, right, rows, W, left_batch, right_batch); break;
    case 2: mirror_pair_launch<2>(st, left, right, rows, W, left_batch, right_batch); break;
    default: mirror_pair_launch<1>(st, left, right, rows, W, left_batch, right_batch);
  }
  AS_CHECK_LAUNCH("as_mirror_pair");
  return AS_OK;
}

template <int V>
static void flip_w_launch(hipStream_t st, const float* src, int64_t rows, int W, float* dst) {
  const int Wq = W / V, xchunks = as_div_up(Wq, LR_THREADS);
  hipLaunchKernelGGL(flip_w_kernel<V>, dim3((unsigned)(rows * xchunks)), dim3(LR_THREADS), 0, st, src, Wq, xchunks, dst);
}

extern "C" int as_flip_w(const float* src, int64_t planes, int H, int W, float* dst, void* stream) {
  AS_CHECK_ARG(src && dst, "as_flip_w: null pointer");
  AS_CHECK_ARG(planes > 0 && planes <= 0x7FFFFFFF && H > 0 && W > 0, "as_flip_w: bad shape (planes %lld, H %d, W %d)",
               (long long)planes, H, W);
  AS_CHECK_ARG(lr_rows_ok((double)planes * H, W), "as_flip_w: %.0f rows of %d elements exceed the grid", (double)planes * H, W);
  const int64_t rows = planes * H;
  const AsRange r[] = {{src, rows * W * 4}, {dst, rows * W * 4}};
  AS_CHECK_ARG(as_disjoint(r, 1, 2), "as_flip_w: dst may not alias src (overlapping ranges)");
  hipStream_t st = (hipStream_t)stream;
  switch (lr_vector_width(W, src, dst)) {
    case 4: flip_w_launch<4>(st, src, rows, W, dst); break;
    case 2: flip_w_launch<2>(st, src, rows, W, dst); break;
    default: flip_w_launch<1>(st, src, rows, W, dst);
  }
  AS_CHECK_LAUNCH("as_flip_w");
  return AS_OK;
}

// ------------------------------------------------------------------------------------------------ the check
struct LrCheckArgs {
  const float* disp[2];            // left, right
  uint8_t* code[2];
  float* valid[2];
  float* diff[2];
  int32_t* counts;
  int H, W, xblocks, mirrored;
  float tol_abs, tol_rel;
};

__global__ __launch_bounds__(LR_THREADS) void lr_check_kernel(LrCheckArgs a) {
  __shared__ int s_count[LR_CODES];
  as_counts_begin(s_count, LR_CODES);

  const int b = blockIdx.y, view = blockIdx.z;                         // view 0: left pixels sampled in the right map, 1: the converse
  const int W = a.W;
  const int mir = a.mirrored ? W - 1 : 0;                              // the right map's element x lives at |mir - x|
  const int tiles = a.H * a.xblocks;                                   // (row, 256 columns) of this image; <= 2^31 - 1 (entry point)
  int mine[LR_CODES] = {0, 0, 0, 0, 0};
  for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int y = (int)(tile / a.xblocks);
    const int x = (int)(tile - (long)y * a.xblocks) * LR_THREADS + threadIdx.x;
    if (x >= W) continue;
    const long row = (long)b * a.H + y;
    const float* L = a.disp[0] + row * W;
    const float* R = a.disp[1] + row * W;
    const float d = view == 0 ? L[x] : R[abs(mir - x)];
    float e = as_qnan();
    int code = 4;
    if (as_disp_usable(d)) {
      const float u = view == 0 ? (float)x - d : (float)x + d;
      code = 3;
      if (view == 0 ? !(u < 0.f) : !(u > (float)(W - 1))) {            // 0 <= u <= W - 1 from here on
        const int i0 = (int)floorf(u);
        const int i1 = min(i0 + 1, W - 1);
        const float t = u - (float)i0;
        const float p = view == 0 ? R[abs(mir - i0)] : L[i0];
        const float q = view == 0 ? R[abs(mir - i1)] : L[i1];
        const float df = q - p;
        const float pr = t * df;
        const float r = t == 0.f ? p : p + pr;
        code = 4;
        if (r - r == 0.f && !(r < 0.f)) {                              // finite and not negative
          e = fabsf(d - r);
          const float rel = a.tol_rel * d;
          const float tol = fmaxf(a.tol_abs, rel);
          code = e <= tol ? 0 : (r > d ? 1 : 2);
        }
      }
    }
    const long at = row * W + x;
    if (a.code[view]) a.code[view][at] = (uint8_t)code;
    if (a.valid[view]) a.valid[view][at] = code == 0 ? 1.f : 0.f;
    if (a.diff[view]) a.diff[view][at] = code >= 3 ? as_qnan() : e;
#pragma unroll
    for (int c = 0; c < LR_CODES; ++c) mine[c] += code == c;
  }
  if (a.counts == nullptr) return;                                     // uniform: no lane waits below
  // as_counts_add, written out: through the helper the compiler hoists the lanes' index arithmetic out of this loop and the tile
  // loop above comes out two instructions longer
#pragma unroll
  for (int c = 0; c < LR_CODES; ++c) {
    int v = mine[c];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(&s_count[c], v);
  }
  as_counts_flush(s_count, LR_CODES, a.counts + (b * 2 + view) * LR_CODES);
}

extern "C" int as_lr_check(const float* disp_l, const float* disp_r, int mirrored, int B, int H, int W, float tol_abs, float tol_rel,
                           uint8_t* code_l, uint8_t* code_r, float* valid_l, float* valid_r, float* diff_l, float* diff_r,
                           int32_t* counts, void* stream) {
  AS_CHECK_ARG(disp_l && disp_r, "as_lr_check: null pointer");
  if (int rc = as_check_images("as_lr_check", B, H, W, true)) return rc;
  AS_CHECK_ARG(W <= LR_MAX_W, "as_lr_check: W %d above 2^24, where a column index is no longer an exact fp32 number", W);
  const int xblocks = as_div_up(W, LR_THREADS);
  AS_CHECK_ARG((int64_t)H * xblocks <= 0x7FFFFFFF, "as_lr_check: %lld tiles an image overflow an int32", (long long)H * xblocks);
  AS_CHECK_ARG(mirrored == 0 || mirrored == 1, "as_lr_check: mirrored %d (0 or 1)", mirrored);
  AS_CHECK_ARG(tol_abs >= 0.f && tol_abs - tol_abs == 0.f && tol_rel >= 0.f && tol_rel - tol_rel == 0.f,
               "as_lr_check: tol_abs %g and tol_rel %g must be finite and not negative", tol_abs, tol_rel);
  AS_CHECK_ARG(code_l || code_r || valid_l || valid_r || diff_l || diff_r || counts, "as_lr_check: no output requested");
  AS_CHECK_ARG(!counts || ((uintptr_t)counts & 3) == 0, "as_lr_check: counts must be 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  if (int rc = as_clear_counts("as_lr_check", counts, B * 2 * LR_CODES, st)) return rc;
  LrCheckArgs a;
  a.disp[0] = disp_l; a.disp[1] = disp_r;
  a.code[0] = code_l; a.code[1] = code_r;
  a.valid[0] = valid_l; a.valid[1] = valid_r;
  a.diff[0] = diff_l; a.diff[1] = diff_r;
  a.counts = counts;
  a.H = H; a.W = W; a.xblocks = xblocks; a.mirrored = mirrored;
  a.tol_abs = tol_abs; a.tol_rel = tol_rel;
  // a workgroup strides over its image's tiles: about LR_CHECK_GROUPS of them in all, so that the five integer atomics each ends
  // with stay a few thousand on one cache line instead of one set per tile
  hipLaunchKernelGGL(lr_check_kernel, as_strided_grid((int64_t)H * xblocks, LR_CHECK_GROUPS, B, 2), dim3(LR_THREADS), 0, st, a);
  AS_CHECK_LAUNCH("as_lr_check");
  return AS_OK;
}

// ------------------------------------------------------------------------------------------------ the fill
struct Last {                       // the last code-0 value of a stretch of the row, if it holds one
  float v;
  int has;
};
static __device__ inline Last then(Last before, Last after) { return after.has ? after : before; }

// One pass of the scan: on entry `own` is the lane's FILL_ITEMS pixels folded together; returns what precedes the lane's first
// pixel (the carry, the waves before, the lanes before) and advances the carry over the whole pass.  s_tot: LR_THREADS/64 slots.
static __device__ inline Last fill_scan_pass(Last own, Last& carry, Last* s_tot) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  Last inc = own;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    Last up;
    up.v = __shfl_up(inc.v, o, 64);
    up.has = __shfl_up(inc.has, o, 64);
    if (lane >= o) inc = then(up, inc);
  }
  Last before;
  before.v = __shfl_up(inc.v, 1, 64);
  before.has = __shfl_up(inc.has, 1, 64);
  if (lane == 0) before.has = 0;
  if (lane == 63) s_tot[wave] = inc;
  __syncthreads();
  Last pre = carry;
#pragma unroll
  for (int w = 0; w < LR_THREADS / 64; ++w) {
    const Last tot = s_tot[w];
    if (w < wave) pre = then(pre, tot);
    carry = then(carry, tot);
  }
  return then(pre, before);
}

__global__ __launch_bounds__(LR_THREADS) void lr_fill_kernel(const float* __restrict__ disp, const uint8_t* __restrict__ code, int W,
                                                             float* out) {
  __shared__ Last s_tot[2][LR_THREADS / 64];                           // by pass parity: one barrier per pass is enough
  __shared__ int s_first;
  const long base = (long)blockIdx.x * W;
  const float* D = disp + base;
  const uint8_t* K = code + base;
  float* O = out + base;
  if (threadIdx.x == 0) s_first = 0x7FFFFFFF;
  __syncthreads();

  const int passes = (W + FILL_SPAN - 1) / FILL_SPAN;
  int first = 0x7FFFFFFF;                                              // the lane's first code-0 pixel
  Last carry = {0.f, 0};
  for (int ps = 0; ps < passes; ++ps) {                                // forward: out = own value, or the nearest one to the left
    const int x0 = ps * FILL_SPAN + threadIdx.x * FILL_ITEMS;
    float v[FILL_ITEMS];
    bool ok[FILL_ITEMS];
    Last own = {0.f, 0};
#pragma unroll
    for (int j = 0; j < FILL_ITEMS; ++j) {
      const int x = x0 + j;
      ok[j] = x < W && K[x] == 0;
      v[j] = x < W ? D[x] : 0.f;
      if (ok[j]) {
        own.v = v[j]; own.has = 1;
        first = min(first, x);
      }
    }
    Last cur = fill_scan_pass(own, carry, s_tot[ps & 1]);
#pragma unroll
    for (int j = 0; j < FILL_ITEMS; ++j) {
      const int x = x0 + j;
      if (ok[j]) { cur.v = v[j]; cur.has = 1; }
      if (x < W) O[x] = cur.has ? cur.v : 0.f;
    }
  }
  if (first != 0x7FFFFFFF) atomicMin(&s_first, first);
  __syncthreads();                                                     // s_first, and this workgroup's stores to `out`
  first = s_first;

  carry = Last{0.f, 0};
  for (int ps = 0; ps < passes; ++ps) {                                // backward: the same scan over x' = W - 1 - x
    const int m0 = ps * FILL_SPAN + threadIdx.x * FILL_ITEMS;
    float v[FILL_ITEMS];
    bool ok[FILL_ITEMS];
    Last own = {0.f, 0};
#pragma unroll
    for (int j = 0; j < FILL_ITEMS; ++j) {
      const int x = W - 1 - (m0 + j);
      ok[j] = x >= 0 && K[x] == 0;
      v[j] = ok[j] ? D[x] : 0.f;
      if (ok[j]) { own.v = v[j]; own.has = 1; }
    }
    Last cur = fill_scan_pass(own, carry, s_tot[(passes + ps) & 1]);
#pragma unroll
    for (int j = 0; j < FILL_ITEMS; ++j) {
      const int x = W - 1 - (m0 + j);
      if (ok[j]) { cur.v = v[j]; cur.has = 1; }
      else if (x >= 0 && cur.has) {                                    // no value to the right: the forward result stands
        const float l = O[x];
        O[x] = (x > first && !(cur.v < l)) ? l : cur.v;               // the smaller; the left one unless the right one is below it
      }
    }
  }
}

extern "C" int as_lr_fill(const float* disp, const uint8_t* code, int B, int H, int W, float* out, void* stream) {
  AS_CHECK_ARG(disp && code && out, "as_lr_fill: null pointer");
  AS_CHECK_ARG(B > 0 && H > 0 && W > 0, "as_lr_fill: bad shape (B %d, H %d, W %d)", B, H, W);
  AS_CHECK_ARG((int64_t)B * H <= 0x7FFFFFFF, "as_lr_fill: %lld rows exceed the grid", (long long)B * H);
  AS_CHECK_ARG(W <= 0x7FFFFFFF - FILL_SPAN, "as_lr_fill: W %d overflows the padded column index", W);
  const int64_t n = (int64_t)B * H * W;
  const AsRange r[] = {{disp, n * 4}, {code, n}, {out, n * 4}};
  AS_CHECK_ARG(as_disjoint(r, 2, 3), "as_lr_fill: out may not alias disp or code (overlapping ranges)");
  hipLaunchKernelGGL(lr_fill_kernel, dim3(B * H), dim3(LR_THREADS), 0, (hipStream_t)stream, disp, code, W, out);
  AS_CHECK_LAUNCH("as_lr_fill");
  return AS_OK;
}
