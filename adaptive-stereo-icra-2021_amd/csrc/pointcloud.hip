// Disparity -> metric depth, organised point cloud and voxel-filtered cloud on the device: the compute of the reference's ROS
// node (ros/stereo_depth_node.py:145-195: F.interpolate to pyramid level s, depth = fx*b/disp, clamp, Open3D's 16-bit depth
// image, pinhole back-projection, voxel_down_sample, x,y,z,rgb records of ros/open3d_to_ros.py:15-22,57), which the node runs
// on the host through .cpu().numpy(), Open3D and a Python loop.
//
// The arithmetic is a CONTRACT (include/adaptive_stereo_hip.h, restated op for op by tests/pointcloud_ref.py): every fp32
// expression is a sequence of single IEEE operations in the written order, so nothing here may contract into an fma, and the
// voxel sums are integers, so a voxel's result does not depend on the order in which its points arrive.
//
//   pointcloud_kernel   one lane per output pixel, lanes along a row: 2x2 mean of the disparity (and colour), depth, quantised
//                       z, x and y, the three voxel indices as one 64-bit key, then the insert into the image's open-addressing
//                       table: atomicCAS on the key (linear probing, at most `slots` probes), 64-bit adds of the coordinates in
//                       2^-16 m, 32-bit adds of the count and the colour.  pointcloud_kernel<true> (as_disp_to_points_gated) is the
//                       same code with one more load and compare per pixel: a confidence below conf_min takes the pixel out
//                       before the index-range check, and the pixels taken out are counted per image (a ballot, one add per wave).
//   finalize_kernel     one lane per slot: occupied slots are compacted into records (one 16-byte store each), one counter add
//                       per wave; every slot it read as occupied is handed back empty, so the next frame starts clean.
//
// One set of atomics per point.  Summing runs of equal adjacent keys inside the wave before the insert (neighbouring pixels of a
// near surface share a voxel) would give identical bits, the sums being integers; it is not built: DESIGN.md §4.
#include "as_common.h"

#pragma clang fp contract(off)

#define PC_EMPTY 0xFFFFFFFFFFFFFFFFull
#define PC_IDX_LIMIT 1048576.f        // 2^20: indices of magnitude >= this are not inserted
#define PC_MAX_BATCH 65535            // images are the grid's y dimension
#define PC_MAX_VOXEL 16.f             // |coord| < 2^20 * 16 m, times 2^16, times < 2^23 points of an image: the sums stay below 2^63

typedef unsigned long long u64;

// Table workspace: per image key[slots] u64 | sum[slots][3] i64 | cnt[slots][4] u32 (count, Sr, Sg, Sb) | dropped u32 (+ 12 bytes), so
// a batch smaller than the one the workspace was sized for uses its first images.
struct PcTable {
  u64* key;
  u64* sum;
  uint32_t* cnt;
  uint32_t* dropped;
};
static inline int64_t pc_image_bytes(int64_t slots) { return slots * 48 + 16; }
__host__ __device__ inline PcTable pc_table(void* table, int64_t slots, int b) {
  PcTable t;
  char* p = static_cast<char*>(table) + (int64_t)b * (slots * 48 + 16);
  t.key = reinterpret_cast<u64*>(p);
  t.sum = reinterpret_cast<u64*>(p + slots * 8);
  t.cnt = reinterpret_cast<uint32_t*>(p + slots * 32);
  t.dropped = reinterpret_cast<uint32_t*>(p + slots * 48);
  return t;
}

struct PcParams {
  int H, W, h, w, s;
  float fb, fxs, fys, cxs, cys, max_depth, depth_scale, depth_trunc, voxel;
};

// mean of the 2x2 source pixels around the centre of output pixel (v, u): ((a + b) + (c + d)) * 0.25
__device__ inline float pc_down(const float* __restrict__ src, int W, int n, int o, int v, int u) {
  const float* p = src + (long)(n * v + o) * W + (n * u + o);
  if (n == 1) return p[0];
  const float a = p[0], b = p[1], c = p[W], d = p[W + 1];
  return ((a + b) + (c + d)) * 0.25f;
}

__device__ inline int pc_colour(float c) {
  const float t = c * 255.f;
  return t >= 255.f ? 255 : (t > 0.f ? (int)t : 0);       // NaN -> 0
}

// One point's contribution: cnt in the top half of cr beside Sr, Sg and Sb in gb
struct PcAdd {
  long long sx, sy, sz;
  uint32_t cr, gb;
};

__device__ inline void pc_insert(const PcTable& t, uint32_t mask, u64 key, const PcAdd& a, bool colour) {
  uint32_t slot = (uint32_t)((key ^ (key >> 33)) * 0xff51afd7ed558ccdull >> 29) & mask;
  for (uint32_t probe = 0; probe <= mask; ++probe) {             // at most `slots` probes: never spins
    const u64 prev = atomicCAS(t.key + slot, PC_EMPTY, key);
    if (prev == PC_EMPTY || prev == key) {
      u64* s = t.sum + (long)slot * 3;
      atomicAdd(s, (u64)a.sx);
      atomicAdd(s + 1, (u64)a.sy);
      atomicAdd(s + 2, (u64)a.sz);
      uint32_t* c = t.cnt + (long)slot * 4;
      atomicAdd(c, a.cr >> 16);
      if (colour) {
        atomicAdd(c + 1, a.cr & 0xFFFFu);
        atomicAdd(c + 2, a.gb >> 16);
        atomicAdd(c + 3, a.gb & 0xFFFFu);
      }
      return;
    }
    slot = (slot + 1) & mask;
  }
  atomicAdd(t.dropped, a.cr >> 16);
}

// GATED: a pixel valid by the depth rules is kept only when conf[b][v][u] >= conf_min (false for a NaN); the ones that fail are
// counted per image, one counter add per wave from a ballot.  Without the flag the code is what it was before the gate existed.
template <bool GATED>
__global__ __launch_bounds__(256) void pointcloud_kernel(const float* __restrict__ disp, const float* __restrict__ rgb, PcParams P,
                                                         float* __restrict__ depth_out, float* __restrict__ xyz_out, void* table,
                                                         long slots, const float* __restrict__ conf, float conf_min,
                                                         int* __restrict__ rejected) {
  const int b = blockIdx.y;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const int hw = P.h * P.w;
  const bool inside = idx < hw;                         // no early return: the wave stays whole for the ballot
  const int n = 1 << P.s, o = n / 2 - 1 + (P.s == 0);   // s = 0: the pixel itself
  const int v = inside ? idx / P.w : 0, u = inside ? idx - v * P.w : 0;
  const long plane = (long)P.H * P.W;

  const float m = pc_down(disp + b * plane, P.W, n, o, v, u);
  const float d = P.fb / m;
  float depth = d != d ? d : fminf(d, P.max_depth);
  depth = depth < 0.f ? 0.f : depth;

  float z;
  bool valid;
  if (P.depth_scale > 0.f) {
    const int q = depth != depth ? 0 : (int)(depth * P.depth_scale);
    z = (float)q / P.depth_scale;
    valid = q != 0 && !(z > P.depth_trunc);
  } else {
    z = depth;
    valid = z > 0.f && z <= P.depth_trunc;
  }
  valid = valid && inside;
  if (GATED) {
    const float c = inside ? conf[(long)b * hw + idx] : 0.f;
    const bool pass = c >= conf_min;                    // false for NaN
    const u64 failed = __ballot(valid && !pass);
    if (rejected && failed && (threadIdx.x & 63) == __ffsll((long long)failed) - 1) atomicAdd(rejected + b, __popcll(failed));
    valid = valid && pass;
  }
  const float x = (((float)u - P.cxs) * z) / P.fxs;
  const float y = (((float)v - P.cys) * z) / P.fys;

  if (inside) {
    if (depth_out) depth_out[(long)b * hw + idx] = depth;
    if (xyz_out) {
      const float nan = as_qnan();
      float* q = xyz_out + (long)b * 3 * hw + idx;
      q[0] = valid ? x : nan;
      q[hw] = valid ? y : nan;
      q[2 * hw] = valid ? z : nan;
    }
  }
  if (!table) return;                                   // (uniform)
  const PcTable T = pc_table(table, slots, b);

  const float fx = floorf(x / P.voxel), fy = floorf(y / P.voxel), fz = floorf(z / P.voxel);
  const bool in_range = fx > -PC_IDX_LIMIT && fx < PC_IDX_LIMIT && fy > -PC_IDX_LIMIT && fy < PC_IDX_LIMIT &&
                        fz > -PC_IDX_LIMIT && fz < PC_IDX_LIMIT;           // false for NaN
  const u64 out_of_range = __ballot(valid && !in_range);
  const int lane = threadIdx.x & 63;
  if (out_of_range && lane == __ffsll((long long)out_of_range) - 1) atomicAdd(T.dropped, (uint32_t)__popcll(out_of_range));
  valid = valid && in_range;

  u64 key = PC_EMPTY;
  PcAdd a = {0, 0, 0, 1u << 16, 0};
  if (valid) {
    key = ((u64)((int)fx + 1048576) << 42) | ((u64)((int)fy + 1048576) << 21) | (u64)((int)fz + 1048576);
    a.sx = llrintf(x * 65536.f);
    a.sy = llrintf(y * 65536.f);
    a.sz = llrintf(z * 65536.f);
  }
  if (rgb) {                                            // (uniform)
    const float* c = rgb + (long)b * 3 * plane;
    a.cr |= (uint32_t)pc_colour(pc_down(c, P.W, n, o, v, u));
    a.gb = ((uint32_t)pc_colour(pc_down(c + plane, P.W, n, o, v, u)) << 16) |
           (uint32_t)pc_colour(pc_down(c + 2 * plane, P.W, n, o, v, u));
  }

  if (valid) pc_insert(T, (uint32_t)(slots - 1), key, a, rgb != nullptr);
}

// records [B][cap] of 16 bytes (x, y, z fp32, R << 16 | G << 8 | B), voxel [B][cap][3], count [B][cap], n [B] (zeroed by the
// entry point in front of this launch), dropped [B]
__global__ __launch_bounds__(256) void finalize_kernel(void* table, long slots, int cap, f32x4* __restrict__ records,
                                                       int* __restrict__ voxel, int* __restrict__ count, int* __restrict__ nvox,
                                                       int* __restrict__ dropped) {
  const int b = blockIdx.y;
  const PcTable T = pc_table(table, slots, b);
  const long slot = (long)blockIdx.x * 256 + threadIdx.x;
  if (slot == 0) {
    dropped[b] = (int)*T.dropped;
    *T.dropped = 0;
  }
  const long at = slot;
  const u64 key = slot < slots ? T.key[at] : PC_EMPTY;
  const bool occupied = key != PC_EMPTY;
  const u64 mask = __ballot(occupied);
  if (!mask) return;                                    // (uniform)
  const int lane = threadIdx.x & 63;
  const int leader = __ffsll((long long)mask) - 1;
  int base = 0;
  if (lane == leader) base = atomicAdd(nvox + b, __popcll(mask));       // one counter add per wave
  base = __shfl(base, leader, 64);
  if (!occupied) return;
  const int row = base + __popcll(mask & ((1ull << lane) - 1));

  u64* s = T.sum + at * 3;
  uint32_t* c = T.cnt + at * 4;
  const long long sx = (long long)s[0], sy = (long long)s[1], sz = (long long)s[2];
  const uint32_t cnt = c[0], sr = c[1], sg = c[2], sb = c[3];
  T.key[at] = PC_EMPTY;                                 // hand the slot back empty
  s[0] = 0; s[1] = 0; s[2] = 0;
  *reinterpret_cast<uint4*>(c) = make_uint4(0, 0, 0, 0);
  if (row >= cap) return;

  const double den = (double)cnt * 65536.0;
  f32x4 r;
  r.x = (float)((double)sx / den);
  r.y = (float)((double)sy / den);
  r.z = (float)((double)sz / den);
  r.w = __uint_as_float(((sr / cnt) << 16) | ((sg / cnt) << 8) | (sb / cnt));
  const long out = (long)b * cap + row;
  records[out] = r;
  voxel[out * 3] = (int)(key >> 42) - 1048576;
  voxel[out * 3 + 1] = (int)((key >> 21) & 0x1FFFFF) - 1048576;
  voxel[out * 3 + 2] = (int)(key & 0x1FFFFF) - 1048576;
  count[out] = (int)cnt;
}

static bool pc_slots_ok(int64_t slots) { return slots >= 64 && slots <= ((int64_t)1 << 30) && (slots & (slots - 1)) == 0; }

extern "C" int64_t as_voxel_table_slots(int64_t points_per_image) {
  if (points_per_image < 0 || points_per_image > ((int64_t)1 << 28)) return -1;
  int64_t s = 1024;
  while (s < 2 * points_per_image) s <<= 1;
  return s;
}

extern "C" int64_t as_voxel_table_bytes(int B, int64_t slots) {
  if (B <= 0 || !pc_slots_ok(slots)) return -1;
  return B * pc_image_bytes(slots);
}

extern "C" int as_voxel_table_clear(void* table, int B, int64_t slots, void* stream) {
  AS_CHECK_ARG(table && ((uintptr_t)table & 15) == 0 && B > 0 && pc_slots_ok(slots),
               "as_voxel_table_clear: bad argument (B %d, slots %lld; the table is 16-byte aligned)", B, (long long)slots);
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipSuccess;
  for (int b = 0; b < B && e == hipSuccess; ++b) {
    const PcTable t = pc_table(table, slots, b);
    e = hipMemsetAsync(t.key, 0xFF, (size_t)slots * 8, st);
    if (e == hipSuccess) e = hipMemsetAsync(t.sum, 0, (size_t)slots * 40 + 16, st);
  }
  if (e != hipSuccess) {
    as_set_error("as_voxel_table_clear: memset failed: %s", hipGetErrorString(e));
    return AS_ERR_LAUNCH;
  }
  return AS_OK;
}

static int pc_disp_to_points(const char* name, const float* disp, const float* rgb, const float* conf, float conf_min, bool gated,
                             int B, int H, int W, int s, const as_depth_camera* cam, float* depth_out, float* xyz_out,
                             float voxel_size, void* table, int64_t slots, int32_t* rejected, void* stream) {
  AS_CHECK_ARG(disp && cam && B > 0 && B <= PC_MAX_BATCH && H > 0 && W > 0 && s >= 0 && s <= 2,
               "%s: bad argument (B %d of at most %d, H %d, W %d, s %d)", name, B, PC_MAX_BATCH, H, W, s);
  const int h = H >> s, w = W >> s;
  AS_CHECK_ARG(h > 0 && w > 0 && (int64_t)B * 3 * H * W < ((int64_t)1 << 40) && (int64_t)H * W < ((int64_t)1 << 30),
               "%s: %dx%d at scale %d has no output pixels, or the frame is too large", name, H, W, s);
  AS_CHECK_ARG(cam->fb == cam->fb && cam->fxs > 0.f && cam->fys > 0.f && cam->cxs == cam->cxs && cam->cys == cam->cys,
               "%s: bad camera (fb %g, fxs %g, fys %g, cxs %g, cys %g)", name, cam->fb, cam->fxs, cam->fys, cam->cxs, cam->cys);
  AS_CHECK_ARG(cam->max_depth > 0.f && cam->depth_scale >= 0.f && cam->depth_trunc > 0.f &&
               (double)cam->max_depth * cam->depth_scale <= 65535.0,
               "%s: max_depth %g * depth_scale %g must fit a 16-bit depth image (and depth_trunc %g be positive)", name,
               cam->max_depth, cam->depth_scale, cam->depth_trunc);
  AS_CHECK_ARG(depth_out || xyz_out || table, "%s: no output requested", name);
  if (gated) AS_CHECK_ARG(conf && conf_min == conf_min, "%s: conf is required and conf_min %g must not be NaN", name, conf_min);
  if (table) {
    AS_CHECK_ARG(voxel_size > 0.f && voxel_size <= PC_MAX_VOXEL, "%s: voxel_size %g outside (0, %g]", name, voxel_size, PC_MAX_VOXEL);
    AS_CHECK_ARG(((uintptr_t)table & 15) == 0, "%s: the table must be 16-byte aligned", name);
    AS_CHECK_ARG(pc_slots_ok(slots) && slots >= (int64_t)h * w,
                 "%s: slots %lld must be a power of two >= 64 and >= h*w = %lld", name, (long long)slots, (long long)h * w);
  }
  PcParams P = {H, W, h, w, s, cam->fb, cam->fxs, cam->fys, cam->cxs, cam->cys, cam->max_depth, cam->depth_scale,
                cam->depth_trunc, voxel_size};
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(as_div_up((long)h * w, 256), B), block(256);
  if (gated) {
    if (rejected) {
      const hipError_t e = hipMemsetAsync(rejected, 0, (size_t)B * 4, st);
      if (e != hipSuccess) {
        as_set_error("%s: memset failed: %s", name, hipGetErrorString(e));
        return AS_ERR_LAUNCH;
      }
    }
    hipLaunchKernelGGL(pointcloud_kernel<true>, grid, block, 0, st, disp, rgb, P, depth_out, xyz_out, table, (long)slots, conf,
                       conf_min, rejected);
  } else {
    hipLaunchKernelGGL(pointcloud_kernel<false>, grid, block, 0, st, disp, rgb, P, depth_out, xyz_out, table, (long)slots,
                       (const float*)nullptr, 0.f, (int*)nullptr);
  }
  AS_CHECK_LAUNCH(name);
  return AS_OK;
}

extern "C" int as_disp_to_points(const float* disp, const float* rgb, int B, int H, int W, int s, const as_depth_camera* cam,
                                 float* depth_out, float* xyz_out, float voxel_size, void* table, int64_t slots, void* stream) {
  return pc_disp_to_points("as_disp_to_points", disp, rgb, nullptr, 0.f, false, B, H, W, s, cam, depth_out, xyz_out, voxel_size, table,
                           slots, nullptr, stream);
}

extern "C" int as_disp_to_points_gated(const float* disp, const float* rgb, const float* conf, float conf_min, int B, int H, int W,
                                       int s, const as_depth_camera* cam, float* depth_out, float* xyz_out, float voxel_size,
                                       void* table, int64_t slots, int32_t* rejected, void* stream) {
  return pc_disp_to_points("as_disp_to_points_gated", disp, rgb, conf, conf_min, true, B, H, W, s, cam, depth_out, xyz_out, voxel_size,
                           table, slots, rejected, stream);
}

extern "C" int as_voxel_cloud_finalize(void* table, int B, int64_t slots, int cap, void* records, int32_t* voxel, int32_t* count,
                                       int32_t* n, int32_t* dropped, void* stream) {
  AS_CHECK_ARG(table && records && voxel && count && n && dropped && B > 0 && B <= PC_MAX_BATCH && cap > 0 && pc_slots_ok(slots) &&
               ((uintptr_t)records & 15) == 0 && ((uintptr_t)table & 15) == 0, "as_voxel_cloud_finalize: bad argument (B %d, slots %lld, cap %d)", B,
               (long long)slots, cap);
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(n, 0, (size_t)B * 4, st);
  if (e != hipSuccess) {
    as_set_error("as_voxel_cloud_finalize: memset failed: %s", hipGetErrorString(e));
    return AS_ERR_LAUNCH;
  }
  hipLaunchKernelGGL(finalize_kernel, dim3(as_div_up(slots, 256), B), dim3(256), 0, st, table, (long)slots,
                     cap, static_cast<f32x4*>(records), voxel, count, n, dropped);
  AS_CHECK_LAUNCH("as_voxel_cloud_finalize");
  return AS_OK;
}
