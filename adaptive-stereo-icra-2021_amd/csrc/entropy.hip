// Per-image Shannon entropy of the 8-bit intensities and of their horizontal differences: the two functions of the reference's
// utils/entropy.py (grayscale_shannon_entropy :11-21, gradient_shannon_entropy :31-44) for a whole batch in one pass, the rows
// appended at a device-side cursor as as_fcs_scores appends its own (csrc/ood.hip).
//
// The arithmetic is a CONTRACT (include/adaptive_stereo_hip.h, restated by tests/entropy_ref.py): integer counts, then per column
// a fixed-order fp64 sum over the 256 bins and one rounding to fp32.  The counts are integer atomics, so the same input gives the
// same bits whatever order the workgroups arrive in.
//
//   image_entropy_kernel  grid (strips, B), 4 waves.  A workgroup owns a strip of rows of one image (a row = W floats of one plane;
//                         the C * H rows of an image are alike).  A wave takes every fourth row of the strip and walks it in chunks
//                         of 64 x 16 bytes laid over the row's 16-byte grid, so every load that lies inside the row is one aligned
//                         16-byte load; the (up to 3) elements of the first and last vector that the row does not cover are not
//                         read and count as invalid.  Four chunks are loaded before the first of them is binned.  The left
//                         neighbour of a lane's first element is the lane below's last one (one lane shift), for lane 0 the
//                         previous chunk's last one: no pixel is read twice.
//                         Each wave has its own pair of 256-bin histograms in LDS.  A lane first joins runs of equal bins among its
//                         four elements; when every valid element of the whole chunk falls into ONE bin (a constant stretch of an
//                         image, the case that would put 64 lanes on one LDS address) a single lane adds the chunk's count.
//                         The workgroup then adds its non-zero bins to the image's 512 counters in the workspace, one atomicAdd
//                         each, and draws a ticket; the workgroup that draws the last ticket of its image reads the counters back,
//                         zeroes them and the ticket for the next call, and writes hist and the score row.
#include "as_common.h"

#pragma clang fp contract(off)

#define ENT_THREADS 256
#define ENT_WAVES (ENT_THREADS / 64)
#define ENT_BINS 256
#define ENT_MAX_BATCH AS_CURSOR_MAX_BATCH   // cursor + b stays inside int32
#define ENT_WG_ELEMS 8192              // elements of a strip, rounded up to whole rows
#define ENT_DEPTH 4                    // 16-byte loads a lane has in flight
#define ENT_WS_WORDS (2 * ENT_BINS + 1)   // per image: gray counts, gradient counts, ticket

// The four elements of vector k of the row's 16-byte grid; elements outside [0, W) come back as NaN (invalid by the contract's
// own rule, so they enter no bin and no difference).  `mis` = how many floats the row start lies past a 16-byte boundary.
__device__ inline f32x4 ent_load(const float* __restrict__ row, int W, int mis, int k, bool active) {
  const float nan = as_qnan();
  f32x4 r = {nan, nan, nan, nan};
  if (!active) return r;
  const int x0 = 4 * k - mis;
  if (x0 >= 0 && x0 + 3 < W) return *reinterpret_cast<const f32x4*>(row + x0);
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (x0 + e >= 0 && x0 + e < W) r[e] = row[x0 + e];
  return r;
}

// Adds the (up to four) bins of every lane, bin < 0 meaning "none", to the wave's histogram h.
__device__ inline void ent_add(uint32_t* __restrict__ h, const int (&bin)[4], int lane) {
  int n = 0, mine = -1;
  bool one = true;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if (bin[e] >= 0) {
      if (mine < 0) mine = bin[e];
      one = one && bin[e] == mine;
      ++n;
    }
  }
  const unsigned long long have = __ballot(n > 0);
  if (have == 0ull) return;                                              // (wave-uniform)
  const int first = __shfl(mine, __ffsll((long long)have) - 1, 64);
  if (__all(one && (n == 0 || mine == first))) {                         // the whole chunk in one bin: one add for the wave
    int total = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) total += __popcll(__ballot(bin[e] >= 0));
    if (lane == 0) atomicAdd(&h[first], (uint32_t)total);
    return;
  }
  int cur = -1, cnt = 0;                                                 // runs of equal bins inside the lane
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if (bin[e] != cur) {
      if (cur >= 0) atomicAdd(&h[cur], (uint32_t)cnt);
      cur = bin[e];
      cnt = 0;
    }
    ++cnt;
  }
  if (cur >= 0) atomicAdd(&h[cur], (uint32_t)cnt);
}

__global__ __launch_bounds__(ENT_THREADS) void image_entropy_kernel(const float* __restrict__ img, int rows, int H, int W,
                                                                    int rows_per_wg, float* __restrict__ scores, int capacity,
                                                                    const int32_t* __restrict__ cursor, uint32_t* __restrict__ hist,
                                                                    uint32_t* __restrict__ ws) {
  // one LDS object: [wave][2][256] counts, later the 2 x 256 fp64 terms; the last word pair holds the "last arriver" flag
  __shared__ double smem_d[ENT_WAVES * ENT_BINS + 1];
  uint32_t* const smem = reinterpret_cast<uint32_t*>(smem_d);
  uint32_t* const flag = smem + 2 * ENT_WAVES * ENT_BINS;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.y;

  for (int i = tid; i < 2 * ENT_WAVES * ENT_BINS; i += ENT_THREADS) smem[i] = 0u;
  __syncthreads();

  uint32_t* const hg = smem + wave * 2 * ENT_BINS;
  uint32_t* const hd = hg + ENT_BINS;
  const float* const image = img + (long)b * rows * W;
  const int r0 = blockIdx.x * rows_per_wg;
  const int r1 = min(rows, r0 + rows_per_wg);
  const int nch = ((W + 3 + 3) / 4 + 63) / 64;                 // chunks of a row at the worst alignment
  const int my_rows = (r1 - r0 - wave + ENT_WAVES - 1) / ENT_WAVES;      // rows r0 + wave, r0 + wave + 4, ...
  const int items = my_rows > 0 ? my_rows * nch : 0;

  // item -> (row, chunk).  ENT_DEPTH items are loaded before the first of them is binned: that many 16-byte loads per lane
  // are in flight, whatever the row length.  A row's pointer, misalignment and vector count are the same for every lane.
  int carry_v = 0;
  bool carry_ok = false;
#pragma unroll 1
  for (int it0 = 0; it0 < items; it0 += ENT_DEPTH) {
    f32x4 xs[ENT_DEPTH];
#pragma unroll
    for (int j = 0; j < ENT_DEPTH; ++j) {
      const int it = it0 + j;
      const bool live = it < items;
      const int ri = live ? it / nch : 0;
      const float* row = image + (long)(r0 + wave + ENT_WAVES * ri) * W;
      const int mis = (int)(((uintptr_t)row >> 2) & 3);
      const int k = (it - ri * nch) * 64 + lane;
      xs[j] = ent_load(row, W, mis, k, live && k < (W + mis + 3) / 4);
    }
#pragma unroll
    for (int j = 0; j < ENT_DEPTH; ++j) {
      if (it0 + j >= items) break;                               // (wave-uniform)
      const f32x4 x = xs[j];
      if ((it0 + j) % nch == 0) carry_ok = false;                // a row's first pixel has no left neighbour

      int v[4];
      bool ok[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float p = 255.0f * x[e];                           // rounded to fp32, then truncated toward zero
        ok[e] = fabsf(p) < 2147483648.0f;                        // false for NaN, +-inf and |p| >= 2^31
        v[e] = ok[e] ? (int)p : 0;
      }
      int left_v = __shfl_up(v[3], 1, 64);
      int left_ok = __shfl_up((int)ok[3], 1, 64);
      if (lane == 0) { left_v = carry_v; left_ok = (int)carry_ok; }
      carry_v = __shfl(v[3], 63, 64);
      carry_ok = __shfl((int)ok[3], 63, 64) != 0;

      int gbin[4], dbin[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        gbin[e] = (ok[e] && v[e] >= 0 && v[e] <= 255) ? v[e] : -1;
        const int lv = e ? v[e - 1] : left_v;
        const bool lok = e ? ok[e - 1] : left_ok != 0;
        const long d = (long)v[e] - (long)lv;
        int q = -1;
        if (ok[e] && lok && d >= -255 && d <= 255) {
          q = ((int)d + 255) * 256 / 510;
          if (q > 255) q = 255;
        }
        dbin[e] = q;
      }
      ent_add(hg, gbin, lane);
      ent_add(hd, dbin, lane);
    }
  }
  __syncthreads();

  // one add per non-zero bin and workgroup
  uint32_t* const wsb = ws + (long)b * ENT_WS_WORDS;
  {
    uint32_t g = 0, d = 0;
#pragma unroll
    for (int w = 0; w < ENT_WAVES; ++w) {
      g += smem[w * 2 * ENT_BINS + tid];
      d += smem[w * 2 * ENT_BINS + ENT_BINS + tid];
    }
    if (g) atomicAdd(&wsb[tid], g);
    if (d) atomicAdd(&wsb[ENT_BINS + tid], d);
  }
  // release: every wave's adds have left it, then one lane publishes them before it draws the ticket
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const uint32_t ticket = __hip_atomic_fetch_add(&wsb[2 * ENT_BINS], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t last = ticket == gridDim.x - 1 ? 1u : 0u;
    if (last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    *flag = last;
  }
  __syncthreads();
  if (*flag == 0u) return;                                     // (uniform)

  // the last workgroup of image b: every shared word is read and re-zeroed with agent-scope accesses
  const uint32_t cg = __hip_atomic_load(&wsb[tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const uint32_t cd = __hip_atomic_load(&wsb[ENT_BINS + tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(&wsb[tid], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(&wsb[ENT_BINS + tid], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (tid == 0) __hip_atomic_store(&wsb[2 * ENT_BINS], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (hist) {
    hist[(long)b * 2 * ENT_BINS + tid] = cg;
    hist[(long)b * 2 * ENT_BINS + ENT_BINS + tid] = cd;
  }
  const double ng = (double)H * (double)W, nd = (double)H * (double)(W - 1);      // the plane's size, whatever C is
  double tg = 0.0, td = 0.0;
  if (cg) { const double p = (double)cg / ng; tg = p * log2(p); }
  if (cd) { const double p = (double)cd / nd; td = p * log2(p); }
  smem_d[tid] = tg;                                            // (every read of the counts in LDS lies before the barriers above)
  smem_d[ENT_BINS + tid] = td;
  __syncthreads();
  if (tid == 0 || tid == 64) {                                 // one lane per column, bins 0..255 in order
    const int col = tid >> 6;
    double s = 0.0;
#pragma unroll 1
    for (int i0 = 0; i0 < ENT_BINS; i0 += 32) {                // 32 terms read at once, added in order
      double t[32];
#pragma unroll
      for (int i = 0; i < 32; ++i) t[i] = smem_d[col * ENT_BINS + i0 + i];
#pragma unroll
      for (int i = 0; i < 32; ++i) s += t[i];
    }
    float out = (float)(-s);
    if (col == 1 && W == 1) out = as_qnan();  // 0 / 0 in the reference's probabilities
    const long r = (long)(cursor ? *cursor : 0) + b;
    if (r >= 0 && r < capacity) scores[2 * r + col] = out;
  }
}

extern "C" int64_t as_image_entropy_workspace(int B) {
  if (B <= 0 || B > ENT_MAX_BATCH) return 0;
  return (((int64_t)B * ENT_WS_WORDS * 4) + 15) & ~(int64_t)15;
}

extern "C" int as_image_entropy(const float* img, int B, int C, int H, int W, float* scores, int capacity, int32_t* cursor,
                                int32_t* dropped, uint32_t* hist, void* workspace, void* stream) {
  AS_CHECK_ARG(img && scores && workspace && B > 0 && B <= ENT_MAX_BATCH && C > 0 && H > 0 && W > 0 &&
                   (int64_t)C * H * W <= ((int64_t)1 << 30),
               "as_image_entropy: bad argument (B %d of at most %d, C %d, H %d, W %d; C*H*W at most 2^30)", B, ENT_MAX_BATCH, C, H, W);
  AS_CHECK_ARG(capacity > 0, "as_image_entropy: capacity %d must be at least 1", capacity);
  AS_CHECK_ARG((((uintptr_t)img | (uintptr_t)scores | (uintptr_t)workspace | (uintptr_t)hist) & 3) == 0,
               "as_image_entropy: img, scores, hist and workspace must be 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int rows = C * H;
  int rows_per_wg = as_div_up(ENT_WG_ELEMS, W);
  if (rows_per_wg < ENT_WAVES) rows_per_wg = ENT_WAVES;
  const int strips = as_div_up(rows, rows_per_wg);
  hipLaunchKernelGGL(image_entropy_kernel, dim3(strips, B), dim3(ENT_THREADS), 0, st, img, rows, H, W, rows_per_wg, scores,
                     capacity, (const int32_t*)cursor, hist, (uint32_t*)workspace);
  AS_CHECK_LAUNCH("as_image_entropy");
  if (cursor || dropped) {
    as_cursor_advance_enqueue(st, cursor, dropped, B, capacity);
    AS_CHECK_LAUNCH("as_image_entropy(cursor)");
  }
  return AS_OK;
}
