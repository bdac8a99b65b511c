// Host side of the generic 32->32 and the thin-input (Cin <= 4 -> 32) convolutions: the argument blocks their entry points
// (conv_entry.hip) hand to the launchers, and the predicates, grids and plans of the kernel families that the route decisions
// of conv_entry.hip are made of.  Host-only declarations: no kernel, no device code.
#pragma once
#include "as_common.h"

// Forward: z = epilogue(conv(x) + bias) (+ residual); stat_*: (mean, M2, count) partials of z, all three or none, written for
// epilogue 0 only; bn_*: stage 1 of the BatchNorm backward that consumes z (the call is then a data gradient).  Unused: null.
struct ConvFwdArgs {
  const float *x, *w, *bias;   // w: as_conv32_pack_weights / as_conv4_pack_weights
  float* z;
  int epilogue;                // 0 raw, 1 lrelu(acc * scale + shift)
  const float *scale, *shift;
  float slope;
  const float* residual;       // in the output geometry
  float *stat_mean, *stat_m2, *stat_cnt;
  const float *bn_z, *bn_scale, *bn_shift, *bn_mean;
  double* bn_partial;          // [workgroups][64]
};
static inline int epilogue_args_ok(int epilogue, const float* sc, const float* sh, const float* sm, const float* s2,
                                   const float* cnt) {
  if (!(epilogue == 0 || (epilogue == 1 && sc && sh))) return 0;
  return (sm == nullptr) == (s2 == nullptr) && (sm == nullptr) == (cnt == nullptr);
}

// Stage 3 of the layer's BatchNorm backward applied to the staged gradient row: g_z from (g_a, z), written to gz_out or, for
// the thin-input layer, projected on the way: h_out[t][p] = sum_co g_z[p][co] * w_proj[t][co] (gz_out null).
struct WgradBnApply {
  const float *z, *scale, *shift, *mean, *coef;
  float* gz_out;
  float slope;
  const float* w_proj;
  float* h_out;
};
// Weight gradient: slabs of dW / db from x and the gradient operand gz (g_a where bn is set)
struct ConvWgradArgs {
  const float *x, *gz;
  float *partial, *partial_db; // [slabs][...], [slabs][32]: laid out by the entry point from its decision's slab count
  const WgradBnApply* bn;      // or null
};

// conv_entry.hip: the geometry checks every convolution entry point starts with (pcl4_input: gin holds 4 floats per pixel)
int check_conv(const as_pcl* gin, const as_pcl* gout, const as_conv_shape* s, const char* who, bool pcl4_input = false);

// The launchers: `who` is the entry point that was called (launch failures are reported under its name).
typedef bool ConvApplicable(const as_pcl* gin, const as_pcl* gout, const as_conv_shape* s);
typedef int ConvFwdLaunch(const ConvFwdArgs&, const as_pcl* gin, const as_pcl* gout, const as_conv_shape* s, const char* who,
                          void* stream);
typedef int ConvWgradLaunch(const ConvWgradArgs&, const as_pcl* gin, const as_pcl* gout, const as_conv_shape* s, const char* who,
                            void* stream);

// conv32_lds.hip: LDS-staged 3x3 stride-1 2-D instance (marks its own profile ids); grid = workgroups = BatchNorm partials
ConvApplicable conv32_lds_applicable;
int conv32_lds_grid(const as_pcl* gout);
ConvFwdLaunch conv32_lds_launch;
int conv32_wgrad_lds_slabs(const as_pcl* gout);
bool conv32_wgrad_bnapply_ok(const as_pcl* gout);      // the form with stage 3 exists for this launch size
ConvWgradLaunch conv32_wgrad_lds_launch;
// conv3d_lds.hip: LDS-staged 3x3x3 stride-1 instance
ConvApplicable conv3d_lds_applicable, conv3d_wgrad_lds_applicable;
int conv3d_lds_grid(const as_pcl* gout);
ConvFwdLaunch conv3d_lds_launch;
int conv3d_wgrad_lds_slabs(const as_pcl* gout);
ConvWgradLaunch conv3d_wgrad_lds_launch;
// conv32_s2.hip: 5x5 stride-2 layers of the feature towers' head, coalesced row staging through wave-private LDS, for maps
// that fill the chip (forward: no epilogue, no residual, no moments)
ConvApplicable conv32_s2_fwd_applicable;
ConvFwdLaunch conv32_s2_fwd_launch;
bool conv32_s2_dgrad_applicable(const as_pcl* ggz, const as_pcl* ggx);
// conv32_mfma.hip: the direct-load kernels.  splitk: a workgroup per 32-voxel tile, its waves splitting the taps
int fill_taps(const as_pcl* gin, const as_conv_shape* s, int* tap_off, const char* who);     // voxel offsets in the padded input
bool conv32_splitk_applies(int ntaps, int64_t M);
int conv32_generic_launch(const ConvFwdArgs&, const as_pcl* gin, const as_pcl* gout, const as_conv_shape* s, bool splitk,
                          const char* who, void* stream);
typedef int DgradS2Launch(const float* gz, const as_pcl* ggz, const float* packed, float* gx, const as_pcl* ggx, const char* who,
                          void* stream);
DgradS2Launch conv32_s2_dgrad_launch, conv32_dgrad_s2_generic_launch;
struct Wgrad32Plan { int T, tap_group, nseg, seg_steps, rows_per_chunk, nchunks; };
Wgrad32Plan conv32_wgrad_plan(const as_pcl* gout, const as_conv_shape* s);
int conv32_wgrad_generic_launch(const ConvWgradArgs&, const as_pcl* gin, const as_pcl* gout, const as_conv_shape* s,
                                const Wgrad32Plan&, const char* who, void* stream);
// conv4_mfma.hip: rows = the 3x3 stride-1 instance over row segments, s2 = the 5x5 stride-2 instance on staged rows
ConvApplicable conv4_rows_applicable, conv4_s2_applicable, conv4_wgrad_rows_applicable;
int conv4_rows_grid(const as_pcl* gout);               // workgroups = BatchNorm partials
int conv4_wgrad_rows_grid(const as_pcl* gout);         // workgroups = slabs of 2 x 1024 floats
ConvFwdLaunch conv4_rows_launch, conv4_s2_fwd_launch, conv4_generic_launch;
ConvWgradLaunch conv4_wgrad_rows_launch;
struct Wgrad4Plan { int nb, nseg, rows_per_chunk, nchunks; };           // nb: 1024-float blocks per slab
Wgrad4Plan conv4_wgrad_plan(const as_pcl* gout, const as_conv_shape* s, bool staged);
int conv4_wgrad_generic_launch(const ConvWgradArgs&, const as_pcl* gin, const as_pcl* gout, const as_conv_shape* s,
                               const Wgrad4Plan&, bool staged, const char* who, void* stream);
// dW[co][c][t] (+)= sum over slabs, db likewise: the tail of every thin-input weight gradient
void conv4_wgrad_reduce_launch(const float* partial, const float* partial_db, int nchunks, int nb, int T, int Cin, float* dW,
                               float* db, int accumulate, void* stream);
