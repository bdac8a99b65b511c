// Host side of the full-resolution 3x3 32->32 layers of the refinement (stereo_net.py:10-18, 33-51, 97): the argument blocks
// their entry points (conv32_layer.hip) hand to the launchers of conv32_act.hip, conv32_wino*.hip and conv32_bwd.hip, the
// tiling of a minimal-filtering launch, and what the launchers share.  Host-only declarations: no kernel, no device code.
#pragma once
#include "as_common.h"
#include <cstdio>
#include <cstdlib>
#include <type_traits>

// Training forward: z = conv(a_prev) + bias with a_prev = lrelu(z_prev * in_scale + in_shift) (+ a_prevprev) formed on the
// way in and written once to a_out; stat_*: (count, mean, M2) partials of z, all three or none.  Unused members are null.
struct LayerFwdArgs {
  const float *z_prev, *a_prevprev, *in_scale, *in_shift;
  float* a_out;
  const float *w, *bias;       // packed for the route: as_conv32_pack_weights (act) / AS_PACK_WINO (minimal filtering)
  float slope;
  float *z, *stat_mean, *stat_m2, *stat_cnt;
};

// Backward: g_z = stage 3 of the layer's BatchNorm backward from (g_a, z), g_x = dgrad(g_z) + g_a, weight / bias gradient
// slabs from (x, g_z), stage-1 sums of the NEXT BatchNorm backward (the layer below) from g_x.  Unused members are null.
struct LayerBwdArgs {
  const float *x, *g_a, *z;
  const float* w;              // the data gradient's filter, packed for the route
  const float *scale, *shift, *mean, *coef;
  float slope;
  const float *next_z, *next_scale, *next_shift, *next_mean;
  float *g_z, *g_x;
  double* next_partial;        // [workgroups][64]
  float *partial, *partial_db; // [slabs][9][32][32], [slabs][32]
};

// Tiling of a minimal-filtering launch: L = log2(dilation) (-1: not 1, 2, 4 or 8), column segments of 64 per row, row pairs
// per (image, segment) summed over the d combs of rows r, r + d, ..  (tests/wino_ref.py restates it for the references).
struct WinoTiling { int L, nseg, pairs; };
inline WinoTiling wino_tiling(const as_pcl* g, const as_conv_shape* s) {
  const int d = s->dil;
  WinoTiling t = {d == 1 ? 0 : d == 2 ? 1 : d == 4 ? 2 : d == 8 ? 3 : -1, (g->W + 63) / 64, 0};
  for (int r = 0; t.L >= 0 && r < d; ++r) t.pairs += ((g->H - r + d - 1) / d + 1) / 2;
  return t;
}

// pick(std::integral_constant<int, L>) for the runtime L of a tiling: the kernel<L> instantiation and what goes with it
template <class F> inline auto wino_by_L(int L, F&& pick) {
  switch (L) {
    case 0: return pick(std::integral_constant<int, 0>());
    case 1: return pick(std::integral_constant<int, 1>());
    case 2: return pick(std::integral_constant<int, 2>());
    default: return pick(std::integral_constant<int, 3>());
  }
}
struct WinoKernel { const void* fn; int lds_bytes; };

// The launchers: `g` is the one padded geometry of every tensor of the layer, `who` the entry point that was called.
typedef int LayerFwdLaunch(const LayerFwdArgs&, const as_pcl* g, const as_conv_shape*, const char* who, void* stream);
typedef int LayerBwdLaunch(const LayerBwdArgs&, const as_pcl* g, const as_conv_shape*, const char* who, void* stream);
typedef bool LayerApplicable(const as_pcl* gin, const as_pcl* gout, const as_conv_shape*);

// conv32_act.hip: the operand formed in LDS, direct 9-tap form
LayerApplicable conv32_act_applicable;
int conv32_act_parts(void);            // workgroups of a launch = BatchNorm partials it writes
LayerFwdLaunch conv32_act_launch;
// conv32_wino.hip: minimal filtering F(2x2, 3x3); MODE 3 is the eval-mode BasicBlock (conv + folded BatchNorm + LeakyReLU
// + skip connection), MODE 2 the first generation of the data gradient (g_z, g_x, next-BatchNorm sums)
LayerApplicable conv32_wino_applicable;
int conv32_wino_parts(void);           // workgroups of a forward launch = BatchNorm partials it writes
LayerFwdLaunch conv32_wino_launch;
int conv32_wino_eval_launch(const float* x, const as_pcl* g, const as_conv_shape* s, const float* wino_w, const float* bias,
                            const float* scale, const float* shift, float slope, int residual, float* out, const char* who,
                            void* stream);
int conv32_wino_dgrad_parts(void);     // workgroups of the data-gradient launch = next-BatchNorm partials it writes
LayerBwdLaunch conv32_wino_dgrad_launch;
// conv32_wino_dgrad.hip: second generation of that data gradient (waves with roles, raw g_a rows kept in LDS for the skip
// connection, rows staged 64 + 2d voxels wide): bit-identical results, the same number of partials
int conv32_wino_dgrad2_parts(void);
LayerBwdLaunch conv32_wino_dgrad2_launch;
// conv32_wino_wgrad.hip: weight / bias gradient slabs from x and g_z
int conv32_wino_wgrad_slabs(void);
LayerBwdLaunch conv32_wino_wgrad_launch;
// conv32_wino_bwd.hip: the whole backward in ONE launch, both gradients side by side in an 8-wave workgroup per CU, g_z never
// leaves the chip; as many slabs as next-BatchNorm partials
int conv32_wino_bwd_fused_parts(void);
LayerBwdLaunch conv32_wino_bwd_fused_launch;
// conv32_bwd.hip: the same in the direct 9-tap form (w: as_conv32_pack_weights, transpose_flip = 1)
LayerApplicable conv32_bwd_fused_applicable;
int conv32_bwd_fused_slabs(void);      // workgroups of a launch = weight-gradient slabs = next-BatchNorm partials
LayerBwdLaunch conv32_bwd_fused_launch;

#include "conv_entry.h"     // check_conv: the geometry checks every convolution entry point starts with

// Diagnostic timing builds (EXTRA=-DWN_TIMING_BUILD / -DFB_TIMING_BUILD / -DBW_TIMING_BUILD): the kernels' per-wave cycle
// counters live in one device buffer per launcher, zeroed before every launch ...
inline long long* as_timing_begin(long long*& buf, size_t bytes, hipStream_t st) {
  if (!buf) (void)hipMalloc(&buf, bytes);
  (void)hipMemsetAsync(buf, 0, bytes, st);
  return buf;
}
// ... and fetched after a launch while `env` is set (synchronises: diagnostic builds only): a malloc'ed host copy that the
// launcher writes to its file and frees, or null
inline void* as_timing_fetch(const char* env, const long long* buf, size_t bytes, hipStream_t st) {
  if (!getenv(env)) return nullptr;
  (void)hipStreamSynchronize(st);
  void* hbuf = malloc(bytes);
  if (hbuf) (void)hipMemcpy(hbuf, buf, bytes, hipMemcpyDeviceToHost);
  return hbuf;
}
