// Entry points of the generic 32->32 convolutions (forward / data gradient / weight gradient, 2-D and 3-D) and of the
// thin-input ones (Cin <= 4 -> 32).  Host code only: the kernels and their launchers are in conv32_lds.hip, conv3d_lds.hip,
// conv32_s2.hip, conv32_mfma.hip and conv4_mfma.hip.  Every entry point does: check, decide, fill an argument block
// (conv_entry.h), launch, and — for a weight gradient — reduce the slabs.  Which kernel takes a layer is decided in ONE function
// per direction and family (conv32_fwd_decide, conv32_wgrad_decide, conv4_fwd_decide, conv4_wgrad_decide): the queries that
// size a caller's buffers and the launches that fill them read the same answer.
#include "conv_entry.h"

static int launched(const char* who, const char* what) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { as_set_error("%s%s: launch failed: %s", who, what, hipGetErrorString(e)); return AS_ERR_LAUNCH; }
  return AS_OK;
}

// pcl4_input: gin describes a PCL4 tensor (4 floats per pixel), which as_pcl_ok's count of 32 floats per voxel must not refuse
int check_conv(const as_pcl* gin, const as_pcl* gout, const as_conv_shape* s, const char* who, bool pcl4_input) {
  AS_CHECK_ARG((pcl4_input ? gin != nullptr : as_pcl_ok(gin)) && as_pcl_ok(gout) && s, "%s: bad geometry", who);
  if (pcl4_input) {            // 2-D only, positive extent, a kernel the tap tables hold
    AS_CHECK_ARG(gin->D == 1 && gout->D == 1 && gin->pd == 0 && gout->pd == 0 && s->kd == 1 && s->pad_d == 0, "%s: 2-D only", who);
    AS_CHECK_ARG(gin->B == gout->B && gin->B > 0 && gin->H > 0 && gin->W > 0, "%s: bad input extent", who);
    const int T = s->kh * s->kw;
    AS_CHECK_ARG(T >= 1 && T <= AS_MAX_TAPS && s->dil >= 1 && s->stride >= 1, "%s: unsupported kernel", who);
  }
  AS_CHECK_ARG(gin->B == gout->B && gin->D == gout->D, "%s: batch/depth mismatch", who);
  // output extent of the convolution
  const int eh = (gin->H + 2 * s->pad_h - s->dil * (s->kh - 1) - 1) / s->stride + 1;
  const int ew = (gin->W + 2 * s->pad_w - s->dil * (s->kw - 1) - 1) / s->stride + 1;
  AS_CHECK_ARG(eh == gout->H && ew == gout->W, "%s: output extent %dx%d != conv result %dx%d", who,
               gout->H, gout->W, eh, ew);
  if (s->kd > 1)
    AS_CHECK_ARG(gin->D + 2 * s->pad_d - s->dil * (s->kd - 1) == gout->D, "%s: depth extent mismatch", who);
  // every tap of every output must land inside the input's halo
  const int reach_h_lo = s->pad_h, reach_w_lo = s->pad_w;
  const int reach_h_hi = (gout->H - 1) * s->stride + s->dil * (s->kh - 1) - s->pad_h - (gin->H - 1);
  const int reach_w_hi = (gout->W - 1) * s->stride + s->dil * (s->kw - 1) - s->pad_w - (gin->W - 1);
  AS_CHECK_ARG(reach_h_lo <= gin->ph && reach_w_lo <= gin->pw && reach_h_hi <= gin->ph && reach_w_hi <= gin->pw,
               "%s: input halo (%d,%d) too small for padding", who, gin->ph, gin->pw);
  if (s->kd > 1) AS_CHECK_ARG(s->pad_d <= gin->pd && s->dil * (s->kd - 1) - s->pad_d <= gin->pd,
                              "%s: input depth halo too small", who);
  return AS_OK;
}

static bool geometry_ok(const as_pcl* gin, const as_pcl* gout, const as_conv_shape* s) { return as_pcl_ok(gin) && as_pcl_ok(gout) && s; }
static int64_t voxels(const as_pcl* g) { return (int64_t)g->B * g->D * g->H * g->W; }
static double conv_flops(const as_pcl* gout, int taps) { return 2.0 * (double)voxels(gout) * 1024.0 * taps; }

// ---- 32->32 forward ------------------------------------------------------------------------------------------------------
// The 5x5 stride-2 layers of the feature head on csrc/conv32_s2.hip (1, default) or on the generic direct-load kernels (0):
// same bits either way (the parity tests compare them); returns the previous setting.
static int g_conv32_s2 = 1;
extern "C" int as_conv32_s2_enable(int on) {
  const int prev = g_conv32_s2;
  if (on == 0 || on == 1) g_conv32_s2 = on;
  return prev;
}

enum class Fwd32 { none, lds2d, lds3d, splitk, staged_s2, direct };
// parts: BatchNorm partials the launch writes (moments, or with stage 1 the sums of the following BatchNorm backward)
struct Fwd32Decision { Fwd32 route; int parts; };
// The LDS kernels first; split-K (small maps) ahead of the staged rows, which take the strided head only on maps that fill
// the chip and write no moments, apply no epilogue and add no residual.  Stage 1 of a BatchNorm backward exists in the 2-D LDS
// kernel alone.
static Fwd32Decision conv32_fwd_decide(const as_pcl* gin, const as_pcl* gout, const as_conv_shape* s, int epilogue,
                                       bool has_residual, bool wants_moments, bool wants_bn_stage1) {
  if (conv32_lds_applicable(gin, gout, s)) return {Fwd32::lds2d, conv32_lds_grid(gout)};
  if (wants_bn_stage1) return {Fwd32::none, 0};
  if (conv3d_lds_applicable(gin, gout, s)) return {Fwd32::lds3d, conv3d_lds_grid(gout)};
  const int64_t M = voxels(gout);
  if (conv32_splitk_applies(s->kd * s->kh * s->kw, M)) return {Fwd32::splitk, as_div_up(M, 32)};     // one partial per 32-voxel tile
  if (epilogue == 0 && !has_residual && !wants_moments && g_conv32_s2 && conv32_s2_fwd_applicable(gin, gout, s))
    return {Fwd32::staged_s2, 0};
  return {Fwd32::direct, as_div_up(M, 128)};
}

extern "C" int as_conv32_num_blocks(const as_pcl* gout) { return as_pcl_ok(gout) ? as_div_up(voxels(gout), 128) : AS_ERR_ARG; }
// Number of BatchNorm partials as_conv32_fwd writes for this configuration.
extern "C" int as_conv32_stat_parts(const as_pcl* gin, const as_pcl* gout, const as_conv_shape* s) {
  return geometry_ok(gin, gout, s) ? conv32_fwd_decide(gin, gout, s, 0, false, true, false).parts : AS_ERR_ARG;
}
// Whether as_conv32_fwd launches conv32_s2_fwd_kernel for epilogue 0 without residual and moments.
extern "C" int as_conv32_s2_fwd_ok(const as_pcl* gin, const as_pcl* gout, const as_conv_shape* s) {
  if (check_conv(gin, gout, s, "as_conv32_s2_fwd_ok")) return AS_ERR_ARG;
  return conv32_fwd_decide(gin, gout, s, 0, false, false, false).route == Fwd32::staged_s2 ? 1 : 0;
}
// Convolution (data gradient) fused with stage 1 of the BatchNorm backward that consumes its output: partials, 0 = unsupported.
extern "C" int as_conv32_bnbwd_parts(const as_pcl* gin, const as_pcl* gout, const as_conv_shape* s) {
  return geometry_ok(gin, gout, s) ? conv32_fwd_decide(gin, gout, s, 0, false, false, true).parts : AS_ERR_ARG;
}

static int conv32_fwd_run(const char* who, const ConvFwdArgs& a, const as_pcl* gin, const as_pcl* gout, const as_conv_shape* s,
                          Fwd32 route, void* stream) {
  if (route == Fwd32::lds2d) return conv32_lds_launch(a, gin, gout, s, who, stream);
  if (route == Fwd32::lds3d) return conv3d_lds_launch(a, gin, gout, s, who, stream);
  hipStream_t st = (hipStream_t)stream;
  as_prof_mark(AS_PROF_CONV32, st, 1, 0.0);
  if (int e = route == Fwd32::staged_s2 ? conv32_s2_fwd_launch(a, gin, gout, s, who, stream)
                                        : conv32_generic_launch(a, gin, gout, s, route == Fwd32::splitk, who, stream)) return e;
  as_prof_mark(AS_PROF_CONV32, st, 0, conv_flops(gout, s->kd * s->kh * s->kw));
  return launched(who, "");
}

extern "C" int as_conv32_fwd(const float* x, const as_pcl* gin, const float* packed_w, const float* bias,
                             float* z, const as_pcl* gout, const as_conv_shape* s,
                             int epilogue, const float* ep_scale, const float* ep_shift, float slope,
                             const float* residual, float* stat_mean, float* stat_m2, float* stat_cnt, void* stream) {
  const char* who = "as_conv32_fwd";
  if (int e = check_conv(gin, gout, s, who)) return e;
  AS_CHECK_ARG(x && packed_w && z, "%s: null pointer", who);
  AS_CHECK_ARG(epilogue_args_ok(epilogue, ep_scale, ep_shift, stat_mean, stat_m2, stat_cnt), "%s: bad epilogue arguments", who);
  const ConvFwdArgs a = {x, packed_w, bias, z, epilogue, ep_scale, ep_shift, slope, residual, stat_mean, stat_m2, stat_cnt};
  const Fwd32Decision d = conv32_fwd_decide(gin, gout, s, epilogue, residual != nullptr, stat_mean != nullptr, false);
  return conv32_fwd_run(who, a, gin, gout, s, d.route, stream);
}

extern "C" int as_conv32_fwd_bnbwd(const float* x, const as_pcl* gin, const float* packed_w, float* z, const as_pcl* gout,
                                   const as_conv_shape* s, const float* residual, const float* bn_z,
                                   const float* bn_scale, const float* bn_shift, const float* bn_mean, float slope,
                                   float* bn_workspace, void* stream) {
  const char* who = "as_conv32_fwd_bnbwd";
  if (int e = check_conv(gin, gout, s, who)) return e;
  AS_CHECK_ARG(x && packed_w && z && bn_z && bn_scale && bn_shift && bn_mean && bn_workspace, "%s: null pointer", who);
  const Fwd32Decision d = conv32_fwd_decide(gin, gout, s, 0, residual != nullptr, false, true);
  AS_CHECK_ARG(d.route != Fwd32::none, "%s: configuration not supported (as_conv32_bnbwd_parts() == 0)", who);
  AS_CHECK_ARG(((uintptr_t)bn_workspace & 7) == 0, "%s: workspace must be 8-byte aligned", who);
  const ConvFwdArgs a = {x, packed_w, nullptr, z, 0, nullptr, nullptr, slope, residual, nullptr, nullptr, nullptr,
                         bn_z, bn_scale, bn_shift, bn_mean, reinterpret_cast<double*>(bn_workspace)};
  return conv32_fwd_run(who, a, gin, gout, s, d.route, stream);
}

// ---- data gradient of the 5x5 stride-2 layers (packing: conv32_mfma.hip) -------------------------------------------------
extern "C" int as_conv32_dgrad_s2(const float* gz, const as_pcl* ggz, const float* w, float* gx, const as_pcl* ggx,
                                  float* workspace, void* stream) {
  AS_CHECK_ARG(w && workspace, "as_conv32_dgrad_s2: null pointer");
  if (int e = as_conv32_dgrad_s2_pack(w, workspace, stream)) return e;
  return as_conv32_dgrad_s2_packed(gz, ggz, workspace, gx, ggx, stream);
}

// Whether as_conv32_dgrad_s2_packed launches conv32_s2_dgrad_kernel (the entry point's own test, switch included).
static bool conv32_s2_dgrad_takes(const as_pcl* ggz, const as_pcl* ggx) {
  return g_conv32_s2 && conv32_s2_dgrad_applicable(ggz, ggx);
}
extern "C" int as_conv32_s2_dgrad_ok(const as_pcl* ggz, const as_pcl* ggx) {
  if (!as_pcl_ok(ggz) || !as_pcl_ok(ggx)) return AS_ERR_ARG;
  return conv32_s2_dgrad_takes(ggz, ggx) ? 1 : 0;
}

extern "C" int as_conv32_dgrad_s2_packed(const float* gz, const as_pcl* ggz, const float* packed, float* gx, const as_pcl* ggx,
                                         void* stream) {
  const char* who = "as_conv32_dgrad_s2";
  AS_CHECK_ARG(as_pcl_ok(ggz) && as_pcl_ok(ggx) && gz && packed && gx, "%s: bad argument", who);
  AS_CHECK_ARG(ggz->D == 1 && ggx->D == 1 && ggz->B == ggx->B, "%s: 2-D tensors of equal batch expected", who);
  AS_CHECK_ARG(ggz->H == (ggx->H - 1) / 2 + 1 && ggz->W == (ggx->W - 1) / 2 + 1,
               "%s: gz extent is not that of a 5x5 stride-2 pad-2 convolution of gx's extent", who);
  AS_CHECK_ARG(ggz->ph >= 1 && ggz->pw >= 1, "%s: gz needs a zero halo of 1", who);
  DgradS2Launch* launch = conv32_s2_dgrad_takes(ggz, ggx) ? conv32_s2_dgrad_launch : conv32_dgrad_s2_generic_launch;
  hipStream_t st = (hipStream_t)stream;
  as_prof_mark(AS_PROF_CONV32, st, 1, 0.0);
  if (int e = launch(gz, ggz, packed, gx, ggx, who, stream)) return e;
  as_prof_mark(AS_PROF_CONV32, st, 0, 2.0 * (double)ggx->B * ggz->H * ggz->W * 1024.0 * 25.0);
  return launched(who, "");
}

// ---- 32->32 weight gradient ----------------------------------------------------------------------------------------------
enum class Wgrad32 { none, lds2d, lds2d_bn3, lds3d, generic };
struct Wgrad32Decision {
  Wgrad32 route;
  int slabs;                   // partial slabs of [T][32][32] + [32] floats the launch writes
  Wgrad32Plan plan;            // T; for the generic kernel also segments per row (0: an LDS kernel), tap group, rows per chunk
};
// The LDS kernels first.  Stage 3 of the layer's BatchNorm backward (the gradient operand arrives as g_a) exists in the 2-D LDS
// kernel's chip-filling form alone.
static Wgrad32Decision conv32_wgrad_decide(const as_pcl* gin, const as_pcl* gout, const as_conv_shape* s, bool wants_bn_stage3) {
  Wgrad32Decision d = {Wgrad32::none, 0, {s->kd * s->kh * s->kw, 0, 0, 0, 0, 0}};
  if (conv32_lds_applicable(gin, gout, s) && gout->pw >= 8) {        // G groups beyond W read 8 zero halo voxels
    if (wants_bn_stage3 && !conv32_wgrad_bnapply_ok(gout)) return d;
    d.route = wants_bn_stage3 ? Wgrad32::lds2d_bn3 : Wgrad32::lds2d;
    d.slabs = conv32_wgrad_lds_slabs(gout);
  } else if (wants_bn_stage3) {
    return d;
  } else if (conv3d_wgrad_lds_applicable(gin, gout, s)) {
    d.route = Wgrad32::lds3d;
    d.slabs = conv3d_wgrad_lds_slabs(gout);
  } else {
    d.route = Wgrad32::generic;
    d.plan = conv32_wgrad_plan(gout, s);
    d.slabs = d.plan.nchunks;
  }
  return d;
}

// Segments per row of conv32_wgrad_kernel for this layer; 0 when an LDS kernel takes it.
extern "C" int as_conv32_wgrad_segments(const as_pcl* gin, const as_pcl* gout, const as_conv_shape* s) {
  if (check_conv(gin, gout, s, "as_conv32_wgrad_segments")) return AS_ERR_ARG;
  return conv32_wgrad_decide(gin, gout, s, false).plan.nseg;
}
extern "C" int64_t as_conv32_wgrad_workspace(const as_pcl* gin, const as_pcl* gout, const as_conv_shape* s) {
  if (!geometry_ok(gin, gout, s)) return -1;
  const Wgrad32Decision d = conv32_wgrad_decide(gin, gout, s, false);
  return (int64_t)d.slabs * d.plan.T * 1024 + (int64_t)d.slabs * 32;
}
extern "C" int as_conv32_wgrad_bnapply_ok(const as_pcl* gin, const as_pcl* gout, const as_conv_shape* s) {
  return geometry_ok(gin, gout, s) ? conv32_wgrad_decide(gin, gout, s, true).route == Wgrad32::lds2d_bn3 : AS_ERR_ARG;
}

static int conv32_wgrad_run(const char* who, ConvWgradArgs a, const as_pcl* gin, const as_pcl* gout, const as_conv_shape* s,
                            const Wgrad32Decision& d, float* dW, float* db, int accumulate, float* workspace, void* stream) {
  const int T = d.plan.T;
  a.partial = workspace; a.partial_db = workspace + (int64_t)d.slabs * T * 1024;
  const int prof_id = d.route == Wgrad32::generic ? AS_PROF_WGRAD32 : d.route == Wgrad32::lds3d ? AS_PROF_WGRAD3D_LDS
                                                                                               : AS_PROF_WGRAD32_LDS;
  hipStream_t st = (hipStream_t)stream;
  as_prof_mark(prof_id, st, 1, 0.0);
  if (int e = d.route == Wgrad32::generic ? conv32_wgrad_generic_launch(a, gin, gout, s, d.plan, who, stream)
              : d.route == Wgrad32::lds3d ? conv3d_wgrad_lds_launch(a, gin, gout, s, who, stream)
                                          : conv32_wgrad_lds_launch(a, gin, gout, s, who, stream)) return e;
  as_prof_mark(prof_id, st, 0, conv_flops(gout, T));
  if (int e = launched(who, "")) return e;
  as_wgrad_reduce_enqueue(st, a.partial, a.partial_db, d.slabs, T, dW, db, accumulate);
  return launched(who, "(reduce)");
}

extern "C" int as_conv32_wgrad(const float* x, const as_pcl* gin, const float* gz, const as_pcl* gout,
                               const as_conv_shape* s, float* dW, float* db, int accumulate, float* workspace,
                               void* stream) {
  const char* who = "as_conv32_wgrad";
  if (int e = check_conv(gin, gout, s, who)) return e;
  AS_CHECK_ARG(x && gz && dW && workspace, "%s: null pointer", who);
  return conv32_wgrad_run(who, {x, gz}, gin, gout, s, conv32_wgrad_decide(gin, gout, s, false), dW, db, accumulate, workspace,
                          stream);
}

extern "C" int as_conv32_wgrad_bnapply(const float* x, const as_pcl* gin, const float* g_a, const float* z,
                                       const as_pcl* gout, const as_conv_shape* s, const float* scale,
                                       const float* shift, const float* mean, const float* coef, float slope,
                                       float* g_z, float* dW, float* db, int accumulate, float* workspace, void* stream) {
  const char* who = "as_conv32_wgrad_bnapply";
  if (int e = check_conv(gin, gout, s, who)) return e;
  AS_CHECK_ARG(x && g_a && z && scale && shift && mean && coef && g_z && dW && workspace, "%s: null pointer", who);
  const Wgrad32Decision d = conv32_wgrad_decide(gin, gout, s, true);
  AS_CHECK_ARG(d.route != Wgrad32::none, "%s: configuration not supported (as_conv32_wgrad_bnapply_ok() == 0)", who);
  const WgradBnApply bn = {z, scale, shift, mean, coef, g_z, slope};
  return conv32_wgrad_run(who, {x, g_a, nullptr, nullptr, &bn}, gin, gout, s, d, dW, db, accumulate, workspace, stream);
}

// ---- thin input, forward -------------------------------------------------------------------------------------------------
static bool g_conv4_s2 = true;
extern "C" int as_conv4_s2_enable(int on) {                // 0 / 1; anything else only reads.  Returns the previous setting.
  const int prev = g_conv4_s2 ? 1 : 0;
  if (on == 0 || on == 1) g_conv4_s2 = on == 1;
  return prev;
}

enum class Fwd4 { rows, staged_s2, generic };
struct Fwd4Decision { Fwd4 route; int parts; };            // parts: BatchNorm partials the launch writes
// The row kernel takes the 3x3 stride-1 layer; the staged rows take the 5x5 stride-2 layer on maps that fill the chip, with a
// plain epilogue and no moments.
static Fwd4Decision conv4_fwd_decide(const as_pcl* gin, const as_pcl* gout, const as_conv_shape* s, int epilogue,
                                     bool wants_moments) {
  if (conv4_rows_applicable(gin, gout, s)) return {Fwd4::rows, conv4_rows_grid(gout)};
  if (g_conv4_s2 && epilogue == 0 && !wants_moments && conv4_s2_applicable(gin, gout, s)) return {Fwd4::staged_s2, 0};
  return {Fwd4::generic, as_div_up((int64_t)gout->B * gout->H * gout->W, 128)};
}

// Number of BatchNorm partials as_conv4_fwd writes for this configuration.
extern "C" int as_conv4_stat_parts(const as_pcl* gin, const as_pcl* gout, const as_conv_shape* s) {
  if (!gin || !gout || !s || !as_pcl_ok(gout)) return AS_ERR_ARG;
  return conv4_fwd_decide(gin, gout, s, 0, true).parts;
}
// Whether as_conv4_fwd launches conv4_s2_fwd_kernel for a plain epilogue without moments.
extern "C" int as_conv4_s2_ok(const as_pcl* gin, const as_pcl* gout, const as_conv_shape* s) {
  if (check_conv(gin, gout, s, "as_conv4_s2_ok", true)) return AS_ERR_ARG;
  return conv4_fwd_decide(gin, gout, s, 0, false).route == Fwd4::staged_s2 ? 1 : 0;
}

extern "C" int as_conv4_fwd(const float* x4, const as_pcl* gin, const float* packed_w, const float* bias,
                            float* z, const as_pcl* gout, const as_conv_shape* s,
                            int epilogue, const float* ep_scale, const float* ep_shift, float slope,
                            float* stat_mean, float* stat_m2, float* stat_cnt, void* stream) {
  const char* who = "as_conv4_fwd";
  if (int e = check_conv(gin, gout, s, who, true)) return e;
  AS_CHECK_ARG(x4 && packed_w && z, "%s: null pointer", who);
  AS_CHECK_ARG(epilogue_args_ok(epilogue, ep_scale, ep_shift, stat_mean, stat_m2, stat_cnt), "%s: bad epilogue arguments", who);
  const ConvFwdArgs a = {x4, packed_w, bias, z, epilogue, ep_scale, ep_shift, slope, nullptr, stat_mean, stat_m2, stat_cnt};
  const Fwd4 route = conv4_fwd_decide(gin, gout, s, epilogue, stat_mean != nullptr).route;
  ConvFwdLaunch* launch = route == Fwd4::rows ? conv4_rows_launch : route == Fwd4::staged_s2 ? conv4_s2_fwd_launch
                                                                                             : conv4_generic_launch;
  if (int e = launch(a, gin, gout, s, who, stream)) return e;
  return launched(who, route == Fwd4::rows ? "(rows)" : route == Fwd4::staged_s2 ? "(5x5 stride 2, staged rows)" : "");
}

// ---- thin input, weight gradient -----------------------------------------------------------------------------------------
enum class Wgrad4 { none, rows, rows_bn3, rows_bn3_proj, staged, generic };
enum class Fused4 { no, bn3, bn3_proj };                   // stage 3 of the layer's BatchNorm backward on the way in
struct Wgrad4Decision {
  Wgrad4 route;
  int nb, nchunks;             // slab layout: nchunks slabs of nb x 1024 floats, then nchunks x 32
  Wgrad4Plan plan;             // staged / generic: segments per row, rows per chunk
  int64_t workspace;           // floats a caller must provide
};
static int64_t slab4_floats(int nchunks, int nb) { return (int64_t)nchunks * nb * 1024 + (int64_t)nchunks * 32; }
// The row kernels take the 3x3 stride-1 layer (alone with stage 3); the 5x5 stride-2 first layer of the feature towers
// goes to the staged rows where the input halo allows.  `workspace` is the largest any plan of this shape needs, whatever the
// switch says and whatever the input halo is: as_conv4_s2_enable may change between the query and the launch, and the query
// knows no input geometry (gin == nullptr: only `workspace` is answered).
static Wgrad4Decision conv4_wgrad_decide(const as_pcl* gin, const as_pcl* gout, const as_conv_shape* s, Fused4 fused) {
  const bool staged_shape = s->kh == 5 && s->kw == 5 && s->stride == 2 && s->dil == 1 && s->pad_h == 2 && s->pad_w == 2;
  const Wgrad4Plan generic = conv4_wgrad_plan(gout, s, false), staged = conv4_wgrad_plan(gout, s, true);
  const int rows_grid = conv4_wgrad_rows_grid(gout);
  Wgrad4Decision d = {Wgrad4::none, 0, 0, generic, slab4_floats(generic.nchunks, generic.nb)};
  if (staged_shape && slab4_floats(staged.nchunks, staged.nb) > d.workspace) d.workspace = slab4_floats(staged.nchunks, staged.nb);
  if (s->kh == 3 && s->kw == 3 && s->stride == 1 && slab4_floats(rows_grid, 2) > d.workspace) d.workspace = slab4_floats(rows_grid, 2);
  if (gin == nullptr) return d;
  if (conv4_wgrad_rows_applicable(gin, gout, s)) {
    d.route = fused == Fused4::bn3_proj ? Wgrad4::rows_bn3_proj : fused == Fused4::bn3 ? Wgrad4::rows_bn3 : Wgrad4::rows;
    d.nb = 2; d.nchunks = rows_grid;
  } else if (fused == Fused4::no) {
    const bool st = g_conv4_s2 && staged_shape && gin->ph >= 2 && gin->pw >= 2;
    d.route = st ? Wgrad4::staged : Wgrad4::generic;
    d.plan = st ? staged : generic;
    d.nb = d.plan.nb; d.nchunks = d.plan.nchunks;
  }
  return d;
}

extern "C" int64_t as_conv4_wgrad_workspace(const as_pcl* gout, const as_conv_shape* s) {
  if (!gout || !s || !as_pcl_ok(gout)) return -1;
  return conv4_wgrad_decide(nullptr, gout, s, Fused4::no).workspace;
}
// Weight gradient fused with stage 3 of the layer's BatchNorm backward (see as_conv32_wgrad_bnapply).
extern "C" int as_conv4_wgrad_bnapply_ok(const as_pcl* gin, const as_pcl* gout, const as_conv_shape* s) {
  if (!gin || !gout || !s || !as_pcl_ok(gout)) return AS_ERR_ARG;
  return conv4_wgrad_decide(gin, gout, s, Fused4::bn3).route == Wgrad4::rows_bn3 ? 1 : 0;
}

// operands_ok: the entry point's own pointers beyond a.x and a.gz
static int conv4_wgrad_run(const char* who, ConvWgradArgs a, bool operands_ok, const as_pcl* gin, const as_pcl* gout,
                           const as_conv_shape* s, int Cin, Fused4 fused, float* dW, float* db, int accumulate, float* workspace,
                           void* stream) {
  if (int e = check_conv(gin, gout, s, who, true)) return e;
  AS_CHECK_ARG(operands_ok && a.x && a.gz && dW && workspace && Cin >= 1 && Cin <= 4, "%s: bad argument", who);
  const Wgrad4Decision d = conv4_wgrad_decide(gin, gout, s, fused);
  AS_CHECK_ARG(d.route != Wgrad4::none, "%s: configuration not supported", who);
  AS_CHECK_ARG(d.nb >= 1 && d.nb <= 4, "%s: kernel too large", who);
  a.partial = workspace; a.partial_db = workspace + (int64_t)d.nchunks * d.nb * 1024;
  const bool rows = d.route != Wgrad4::staged && d.route != Wgrad4::generic;
  if (int e = rows ? conv4_wgrad_rows_launch(a, gin, gout, s, who, stream)
                   : conv4_wgrad_generic_launch(a, gin, gout, s, d.plan, d.route == Wgrad4::staged, who, stream)) return e;
  if (int e = launched(who, rows ? "(rows)" : "")) return e;
  conv4_wgrad_reduce_launch(a.partial, a.partial_db, d.nchunks, d.nb, s->kh * s->kw, Cin, dW, db, accumulate, stream);
  return launched(who, "(reduce)");
}

extern "C" int as_conv4_wgrad(const float* x4, const as_pcl* gin, const float* gz, const as_pcl* gout,
                              const as_conv_shape* s, int Cin, float* dW, float* db, int accumulate, float* workspace,
                              void* stream) {
  return conv4_wgrad_run("as_conv4_wgrad", {x4, gz}, true, gin, gout, s, Cin, Fused4::no, dW, db, accumulate, workspace, stream);
}

extern "C" int as_conv4_wgrad_bnapply(const float* x4, const as_pcl* gin, const float* g_a, const float* z,
                                      const as_pcl* gout, const as_conv_shape* s, int Cin, const float* scale,
                                      const float* shift, const float* mean, const float* coef, float slope, float* g_z,
                                      float* dW, float* db, int accumulate, float* workspace, void* stream) {
  const WgradBnApply bn = {z, scale, shift, mean, coef, g_z, slope};
  return conv4_wgrad_run("as_conv4_wgrad_bnapply", {x4, g_a, nullptr, nullptr, &bn}, z && scale && shift && mean && coef && g_z,
                         gin, gout, s, Cin, Fused4::bn3, dW, db, accumulate, workspace, stream);
}

// As as_conv4_wgrad_bnapply, but g_z is not written: the nine per-tap projections h[t][p] = sum_co g_z[p][co] * w_proj[t][co]
// are ([B][9][H][W]), which is all a following 3x3 32->1 data gradient needs (as_tap_gather sums the nine shifted planes).
extern "C" int as_conv4_wgrad_bnapply_proj(const float* x4, const as_pcl* gin, const float* g_a, const float* z,
                                           const as_pcl* gout, const as_conv_shape* s, int Cin, const float* scale,
                                           const float* shift, const float* mean, const float* coef, float slope,
                                           const float* w_proj, float* h, float* dW, float* db, int accumulate,
                                           float* workspace, void* stream) {
  const WgradBnApply bn = {z, scale, shift, mean, coef, nullptr, slope, w_proj, h};
  return conv4_wgrad_run("as_conv4_wgrad_bnapply_proj", {x4, g_a, nullptr, nullptr, &bn},
                         z && scale && shift && mean && coef && w_proj && h, gin, gout, s, Cin, Fused4::bn3_proj, dW, db, accumulate,
                         workspace, stream);
}
