// Entry points of the full-resolution 3x3 32->32 layers of the refinement (stereo_net.py:10-18, 33-51, 97): training forward
// with the previous layer's BatchNorm + LeakyReLU (+ skip) formed on the way in, eval-mode BasicBlock, and the backward in
// one, two or three launches.  Host code only: the kernels are in conv32_act.hip, conv32_wino*.hip and conv32_bwd.hip.
// Every entry point fills an argument block (conv32_layer.h), runs the one check below with ITS rules, launches, and — where
// it produced weight-gradient slabs — ends in reduce_slabs.
#include "conv32_layer.h"
#include <initializer_list>

struct AliasPair { const void *a, *b; };
// What an entry point refuses, tested in this order; a rule an entry point does not have is left empty / null.
struct LayerRules {
  LayerApplicable* applicable; const char* ok_query;   // "configuration not supported (<ok_query>() == 0)"
  std::initializer_list<const void*> required;         // each must be non-null
  std::initializer_list<const void*> moments;          // all null or none
  const void* aligned8;                                // the next BatchNorm's fp64 partials
  const float* slope;                                  // must lie in (0, 1)
  const char* alias_rule; std::initializer_list<AliasPair> alias;
};

static int layer_check(const char* who, const as_pcl* gin, const as_pcl* gout, const as_conv_shape* s, const LayerRules& r) {
  if (int e = check_conv(gin, gout, s, who)) return e;
  for (const void* p : r.required) AS_CHECK_ARG(p != nullptr, "%s: null pointer", who);
  int given = 0;
  for (const void* p : r.moments) given += p != nullptr;
  AS_CHECK_ARG(given == 0 || given == (int)r.moments.size(), "%s: pass all three moment arrays or none", who);
  AS_CHECK_ARG(r.applicable(gin, gout, s), "%s: configuration not supported (%s() == 0)", who, r.ok_query);
  AS_CHECK_ARG(((uintptr_t)r.aligned8 & 7) == 0, "%s: the BatchNorm workspace must be 8-byte aligned", who);
  AS_CHECK_ARG(r.slope == nullptr || (*r.slope > 0.f && *r.slope < 1.f), "%s: slope must lie in (0, 1)", who);
  for (const AliasPair& p : r.alias) AS_CHECK_ARG(p.a != p.b, "%s: %s", who, r.alias_rule);
  return AS_OK;
}

// One launch between the marks of the measurement hook.  (ALGORITHMIC flops: `passes` times the direct form's 9 taps — what
// the layer computes, not the 4 products per pixel minimal filtering executes.)
template <class Args>
static int timed_launch(int (*launch)(const Args&, const as_pcl*, const as_conv_shape*, const char*, void*), const Args& a,
                        const as_pcl* g, const as_conv_shape* s, const char* who, int prof_id, double passes, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  as_prof_mark(prof_id, st, 1, 0.0);
  if (int e = launch(a, g, s, who, stream)) return e;
  as_prof_mark(prof_id, st, 0, passes * 2.0 * (double)g->B * g->H * g->W * 1024.0 * 9);
  AS_CHECK_LAUNCH(who);
  return AS_OK;
}

// The tail of every weight gradient: workspace = [slabs][9][32][32] weight slabs, then [slabs][32] bias slabs
static float* slab_db(float* workspace, int slabs) { return workspace ? workspace + (int64_t)slabs * 9 * 1024 : nullptr; }
static int64_t slab_floats(int slabs) { return (int64_t)slabs * (9 * 1024 + 32); }
static int reduce_slabs(const char* who, float* workspace, int slabs, float* dW, float* db, int accumulate, void* stream) {
  as_wgrad_reduce_enqueue((hipStream_t)stream, workspace, slab_db(workspace, slabs), slabs, 9, dW, db, accumulate);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { as_set_error("%s(reduce): launch failed: %s", who, hipGetErrorString(e)); return AS_ERR_LAUNCH; }
  return AS_OK;
}

static int layer_ok(LayerApplicable* applicable, const as_pcl* gin, const as_pcl* gout, const as_conv_shape* s) {
  if (!as_pcl_ok(gin) || !as_pcl_ok(gout) || !s) return AS_ERR_ARG;
  return applicable(gin, gout, s) ? 1 : 0;
}

// ---- training forward: the operand is the PREVIOUS layer's output, formed on the way in from that layer's pre-activation,
// BatchNorm affine and skip input; direct form (conv32_act.hip) or minimal filtering F(2x2, 3x3) (conv32_wino.hip: 4 matrix
// products per output pixel instead of 9; w: as_conv32_wino_pack_weights or a batch job of kind AS_PACK_WINO)
static int layer_fwd(const char* who, const LayerFwdArgs& a, const as_pcl* gin, const as_pcl* gout, const as_conv_shape* s,
                     LayerApplicable* applicable, const char* ok_query, LayerFwdLaunch* launch, int prof_id, void* stream) {
  if (int e = layer_check(who, gin, gout, s,
                          {applicable, ok_query, {a.z_prev, a.in_scale, a.in_shift, a.a_out, a.w, a.z},
                           {a.stat_mean, a.stat_m2, a.stat_cnt}, nullptr, &a.slope, "outputs must not alias inputs or each other",
                           {{a.a_out, a.z_prev}, {a.a_out, a.a_prevprev}, {a.z, a.z_prev}, {a.z, a.a_out}, {a.z, a.a_prevprev}}}))
    return e;
  return timed_launch(launch, a, gout, s, who, prof_id, 1.0, stream);
}

extern "C" int as_conv32_act_ok(const as_pcl* gin, const as_pcl* gout, const as_conv_shape* s) {
  return layer_ok(conv32_act_applicable, gin, gout, s);
}
extern "C" int as_conv32_act_parts(void) { return conv32_act_parts(); }
extern "C" int as_conv32_act_fwd(const float* z_prev, const float* a_prevprev, const float* in_scale, const float* in_shift,
                                 float* a_out, const as_pcl* gin, const float* packed_w, const float* bias, float slope,
                                 float* z, const as_pcl* gout, const as_conv_shape* s, float* stat_mean, float* stat_m2,
                                 float* stat_cnt, void* stream) {
  const LayerFwdArgs a = {z_prev, a_prevprev, in_scale, in_shift, a_out, packed_w, bias, slope, z, stat_mean, stat_m2, stat_cnt};
  return layer_fwd("as_conv32_act_fwd", a, gin, gout, s, conv32_act_applicable, "as_conv32_act_ok", conv32_act_launch,
                   AS_PROF_CONV_ACT, stream);
}

extern "C" int as_conv32_wino_ok(const as_pcl* gin, const as_pcl* gout, const as_conv_shape* s) {
  return layer_ok(conv32_wino_applicable, gin, gout, s);
}
extern "C" int as_conv32_wino_parts(void) { return conv32_wino_parts(); }
extern "C" int as_conv32_wino_fwd(const float* z_prev, const float* a_prevprev, const float* in_scale, const float* in_shift,
                                  float* a_out, const as_pcl* gin, const float* wino_w, const float* bias, float slope,
                                  float* z, const as_pcl* gout, const as_conv_shape* s, float* stat_mean, float* stat_m2,
                                  float* stat_cnt, void* stream) {
  const LayerFwdArgs a = {z_prev, a_prevprev, in_scale, in_shift, a_out, wino_w, bias, slope, z, stat_mean, stat_m2, stat_cnt};
  return layer_fwd("as_conv32_wino_fwd", a, gin, gout, s, conv32_wino_applicable, "as_conv32_wino_ok", conv32_wino_launch,
                   AS_PROF_WINO_FWD, stream);
}

// Eval-mode BasicBlock by minimal filtering: out = lrelu((conv(x) + bias) * scale + shift) (+ x).  One read of x (the skip
// connection comes out of the staged rows), one write.
extern "C" int as_conv32_wino_eval(const float* x, const as_pcl* g, const as_conv_shape* s, const float* wino_w, const float* bias,
                                   const float* scale, const float* shift, float slope, int residual, float* out, void* stream) {
  const char* who = "as_conv32_wino_eval";
  if (int e = layer_check(who, g, g, s, {conv32_wino_applicable, "as_conv32_wino_ok", {x, wino_w, scale, shift, out}, {}, nullptr,
                                         &slope, "out must not alias x", {{out, x}}})) return e;
  hipStream_t st = (hipStream_t)stream;
  as_prof_mark(AS_PROF_WINO_FWD, st, 1, 0.0);
  if (int e = conv32_wino_eval_launch(x, g, s, wino_w, bias, scale, shift, slope, residual, out, who, stream)) return e;
  as_prof_mark(AS_PROF_WINO_FWD, st, 0, 2.0 * (double)g->B * g->H * g->W * 1024.0 * 9);
  AS_CHECK_LAUNCH(who);
  return AS_OK;
}

// ---- backward by minimal filtering, two launches: data gradient F(2x2, 3x3) with stage 3 of the BatchNorm backward on the
// way in (g_z written once), skip connection and next-BatchNorm sums in the epilogue; then weight / bias gradient F(3x3, 2x2)
// from x and g_z.  Arguments as as_conv32_bwd_fused, plus g_z (a PCL buffer of the layer's geometry).
extern "C" int as_conv32_wino_bwd_parts(void) { return conv32_wino_dgrad_parts(); }
// Which data-gradient kernel as_conv32_wino_bwd_data launches: 2 (default) = conv32_wino_dgrad.hip where it is the faster one
// (dilation 1, 2, 4), 1 = conv32_wino.hip MODE 2 everywhere, 3 = conv32_wino_dgrad.hip everywhere (its dilation-8 instantiation
// is slower than generation 1 and only here for the parity tests).  All write the same bits; returns the previous setting.
static int g_wino_dgrad_generation = 2;
extern "C" int as_conv32_wino_bwd_generation(int generation) {
  const int prev = g_wino_dgrad_generation;
  if (generation >= 1 && generation <= 3) g_wino_dgrad_generation = generation;
  return prev;
}
extern "C" int64_t as_conv32_wino_bwd_workspace(void) { return slab_floats(conv32_wino_wgrad_slabs()); }

// The two halves separately (a caller may run the weight gradient on another stream: nothing but the step's final slab
// reduction waits for it) ...
extern "C" int as_conv32_wino_bwd_data(const float* g_a, const float* z, const as_pcl* g, const as_conv_shape* s,
                                       const float* wino_wt, const float* scale, const float* shift, const float* mean,
                                       const float* coef, float slope, const float* next_z, const float* next_scale,
                                       const float* next_shift, const float* next_mean, float* g_z, float* g_x,
                                       float* next_bn_workspace, void* stream) {
  const char* who = "as_conv32_wino_bwd_data";
  const LayerBwdArgs a = {nullptr, g_a, z, wino_wt, scale, shift, mean, coef, slope, next_z, next_scale, next_shift, next_mean,
                          g_z, g_x, reinterpret_cast<double*>(next_bn_workspace), nullptr, nullptr};
  if (int e = layer_check(who, g, g, s,
                          {conv32_wino_applicable, "as_conv32_wino_ok",
                           {g_a, z, wino_wt, scale, shift, mean, coef, next_z, next_scale, next_shift, next_mean, g_z, g_x,
                            next_bn_workspace}, {}, next_bn_workspace, &slope, "outputs must not alias inputs or each other",
                           {{g_x, g_a}, {g_x, z}, {g_z, g_a}, {g_z, z}, {g_z, g_x}, {g_z, next_z}, {g_x, next_z}}})) return e;
  if (conv32_wino_dgrad2_parts() != conv32_wino_dgrad_parts()) { as_set_error("%s: partial counts differ", who); return AS_ERR_ARG; }
  // (generation 2 wins for dilation 1, 2, 4 — 286 / 269 / 268 us against 343 / 300 / 287 at 4 pairs — and loses at 8, where
  //  only one of its three raw-row slots fits the LDS: 335 against 288; profiles/r04_b_dgrad_generations.txt)
  const bool gen2 = g_wino_dgrad_generation == 3 || (g_wino_dgrad_generation == 2 && s->dil <= 4);
  return timed_launch(gen2 ? conv32_wino_dgrad2_launch : conv32_wino_dgrad_launch, a, g, s, who, AS_PROF_WINO_DGRAD, 1.0, stream);
}

extern "C" int as_conv32_wino_bwd_filter(const float* x, const float* g_z, const as_pcl* g, const as_conv_shape* s, float* dW,
                                         float* db, int accumulate, float* workspace, void* stream) {
  const char* who = "as_conv32_wino_bwd_filter";
  if (int e = layer_check(who, g, g, s, {conv32_wino_applicable, "as_conv32_wino_ok", {x, g_z, dW, workspace}, {}, nullptr, nullptr,
                                         nullptr, {}})) return e;
  const int slabs = conv32_wino_wgrad_slabs();
  LayerBwdArgs a = {};
  a.x = x; a.g_z = const_cast<float*>(g_z); a.partial = workspace; a.partial_db = slab_db(workspace, slabs);
  if (int e = timed_launch(conv32_wino_wgrad_launch, a, g, s, who, AS_PROF_WINO_WGRAD, 1.0, stream)) return e;
  return reduce_slabs(who, workspace, slabs, dW, db, accumulate, stream);
}

// ... and both on one stream
extern "C" int as_conv32_wino_bwd(const float* x, const as_pcl* gin, const float* g_a, const float* z, const as_pcl* gout,
                                  const as_conv_shape* s, const float* wino_wt, const float* scale, const float* shift,
                                  const float* mean, const float* coef, float slope, const float* next_z,
                                  const float* next_scale, const float* next_shift, const float* next_mean, float* g_z,
                                  float* g_x, float* dW, float* db, int accumulate, float* next_bn_workspace,
                                  float* workspace, void* stream) {
  // (both launches below take gout alone: x laid out in another padded geometry would be read with the wrong strides)
  if (int e = layer_check("as_conv32_wino_bwd", gin, gout, s,
                          {conv32_wino_applicable, "as_conv32_wino_ok", {x, dW, workspace}, {}, nullptr, nullptr,
                           "outputs must not alias inputs or each other", {{g_x, x}, {g_z, x}}})) return e;
  if (int e = as_conv32_wino_bwd_data(g_a, z, gout, s, wino_wt, scale, shift, mean, coef, slope, next_z, next_scale, next_shift,
                                      next_mean, g_z, g_x, next_bn_workspace, stream)) return e;
  return as_conv32_wino_bwd_filter(x, g_z, gout, s, dW, db, accumulate, workspace, stream);
}

// ---- the whole backward in ONE launch: stage 3 of the layer's BatchNorm backward, data gradient + skip connection, weight /
// bias gradient, stage 1 of the next BatchNorm backward.  By minimal filtering (conv32_wino_bwd.hip: data and weight gradient
// side by side in an 8-wave workgroup per CU, g_z never leaves the chip — 5 tensor passes instead of 7; g_x bit-identical to
// the two-launch form) or in the direct form (conv32_bwd.hip), which checks no slope.  Arguments of as_conv32_wino_bwd
// without g_z.
extern "C" int as_conv32_wino_bwd_fused_parts(void) { return conv32_wino_bwd_fused_parts(); }
extern "C" int64_t as_conv32_wino_bwd_fused_workspace(void) { return slab_floats(conv32_wino_bwd_fused_parts()); }
extern "C" int as_conv32_wino_bwd_fused(const float* x, const as_pcl* gin, const float* g_a, const float* z, const as_pcl* gout,
                                        const as_conv_shape* s, const float* wino_wt, const float* scale, const float* shift,
                                        const float* mean, const float* coef, float slope, const float* next_z,
                                        const float* next_scale, const float* next_shift, const float* next_mean, float* g_x,
                                        float* dW, float* db, int accumulate, float* next_bn_workspace, float* workspace,
                                        void* stream) {
  const char* who = "as_conv32_wino_bwd_fused";
  const int slabs = conv32_wino_bwd_fused_parts();
  const LayerBwdArgs a = {x, g_a, z, wino_wt, scale, shift, mean, coef, slope, next_z, next_scale, next_shift, next_mean, nullptr, g_x,
                          reinterpret_cast<double*>(next_bn_workspace), workspace, slab_db(workspace, slabs)};
  if (int e = layer_check(who, gin, gout, s,
                          {conv32_wino_applicable, "as_conv32_wino_ok",
                           {x, g_a, z, wino_wt, scale, shift, mean, coef, next_z, next_scale, next_shift, next_mean, g_x, dW,
                            next_bn_workspace, workspace}, {}, next_bn_workspace, &slope, "g_x must not alias an input",
                           {{g_x, g_a}, {g_x, z}, {g_x, x}, {g_x, next_z}}})) return e;
  if (int e = timed_launch(conv32_wino_bwd_fused_launch, a, gout, s, who, AS_PROF_WINO_BWD, 2.0, stream)) return e;   // dgrad + wgrad
  return reduce_slabs(who, workspace, slabs, dW, db, accumulate, stream);
}

extern "C" int as_conv32_bwd_fused_ok(const as_pcl* gin, const as_pcl* gout, const as_conv_shape* s) {
  return layer_ok(conv32_bwd_fused_applicable, gin, gout, s);
}
extern "C" int as_conv32_bwd_fused_parts(void) { return conv32_bwd_fused_slabs(); }
extern "C" int64_t as_conv32_bwd_fused_workspace(void) { return slab_floats(conv32_bwd_fused_slabs()); }
extern "C" int as_conv32_bwd_fused(const float* x, const as_pcl* gin, const float* g_a, const float* z, const as_pcl* gout,
                                   const as_conv_shape* s, const float* packed_wt, const float* scale, const float* shift,
                                   const float* mean, const float* coef, float slope, const float* next_z,
                                   const float* next_scale, const float* next_shift, const float* next_mean, float* g_x,
                                   float* dW, float* db, int accumulate, float* next_bn_workspace, float* workspace,
                                   void* stream) {
  const char* who = "as_conv32_bwd_fused";
  const int slabs = conv32_bwd_fused_slabs();
  const LayerBwdArgs a = {x, g_a, z, packed_wt, scale, shift, mean, coef, slope, next_z, next_scale, next_shift, next_mean, nullptr,
                          g_x, reinterpret_cast<double*>(next_bn_workspace), workspace, slab_db(workspace, slabs)};
  if (int e = layer_check(who, gin, gout, s,
                          {conv32_bwd_fused_applicable, "as_conv32_bwd_fused_ok",
                           {x, g_a, z, packed_wt, scale, shift, mean, coef, next_z, next_scale, next_shift, next_mean, g_x, dW,
                            next_bn_workspace, workspace}, {}, next_bn_workspace, nullptr, "g_x must not alias an input",
                           {{g_x, g_a}, {g_x, x}, {g_x, z}}})) return e;
  if (int e = timed_launch(conv32_bwd_fused_launch, a, gout, s, who, AS_PROF_BWD_FUSED, 2.0, stream)) return e;       // dgrad + wgrad
  return reduce_slabs(who, workspace, slabs, dW, db, accumulate, stream);
}
