/*
 * adaptive_stereo_hip.h — C ABI of libadaptive_stereo_hip.so (gfx950 / MI355X).
 *
 * This is the drop-in boundary for the StereoNet online-adaptation hot path
 * (SURVEY.md §8).  The reference (miloknowles/adaptive-stereo-icra-2021) is pure
 * Python/PyTorch and has no FFI of its own: the interfaces these entry points
 * replace are the PyTorch op sequences inside the reference's nn.Module.forward()
 * bodies and loss functions, cited per function below (paths relative to the
 * reference root).  INTEGRATION.md shows the ctypes binding a maintainer of the
 * reference would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to fp32 unless stated otherwise;
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it, no
 *     entry point synchronises, allocates or frees (safe under hipGraph capture);
 *   - the caller owns every buffer; nothing is retained after return;
 *   - return value: 0 on success, negative on error; as_last_error() returns a
 *     thread-local description of the last failure;
 *   - "NCHW"/"NCDHW" are the reference's contiguous PyTorch layouts;
 *   - "PCL" (padded channel-last) is this library's internal activation layout:
 *       float buf[B][D+2*pd][H+2*ph][W+2*pw][32]
 *     with a zero halo that kernels never write.  Halo zeros implement the
 *     convolutions' zero padding, so no kernel needs bounds predicates, and the
 *     32 channels of a voxel are one aligned 128-byte line.  2-D maps use D=1, pd=0.
 */
#ifndef ADAPTIVE_STEREO_HIP_H_
#define ADAPTIVE_STEREO_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AS_CHANNELS 32
#define AS_MAX_TAPS 32

/* Geometry of one PCL tensor. */
typedef struct as_pcl {
  int32_t B, D, H, W;     /* logical extent */
  int32_t pd, ph, pw;     /* halo width on each side of D, H, W */
} as_pcl;

/* Shape of a 32->32 convolution over PCL tensors. kd=1 for 2-D. */
typedef struct as_conv_shape {
  int32_t kd, kh, kw;     /* kernel extent */
  int32_t pad_d, pad_h, pad_w;   /* logical zero padding (must be <= input halo) */
  int32_t dil;            /* dilation on H and W (and D when kd>1) */
  int32_t stride;         /* stride on H and W (D always 1) */
} as_conv_shape;

const char* as_last_error(void);
int  as_version(void);
/* Number of floats a PCL tensor occupies. */
int64_t as_pcl_numel(const as_pcl* g);

/* ---- a2: difference cost volume — stereo_net.py:173-184 -------------------
 * vol[b,d,y,x,c] = L[b,c,y,x] - R[b,c,y,x-d]  (x >= d), else 0.
 * L, R: NCHW [B,32,H,W].  vol: PCL {B,D,H,W}.  bwd adds nothing: it overwrites gL, gR. */
int as_cost_volume_fwd(const float* L, const float* R, float* vol, const as_pcl* g, void* stream);
int as_cost_volume_bwd(const float* gvol, float* gL, float* gR, const as_pcl* g, void* stream);

/* ---- a3 (and a1/a7 32->32 convs): fp32-MFMA implicit-GEMM convolution ------
 * Replaces nn.Conv3d(32,32,3,padding=1) of convbn_3d (stereo_net.py:21-30,185-186)
 * and the 32->32 nn.Conv2d layers (stereo_net.py:10-18).
 *
 * as_conv32_pack_weights: w is the PyTorch weight [32(out)][32(in)][kd][kh][kw];
 *   packed is [taps][2][32][16] floats in MFMA operand order.  transpose_flip=1
 *   produces the weights of the data-gradient convolution (in/out swapped, taps
 *   mirrored), so dgrad is the same kernel as forward.
 * as_conv32_fwd: z = conv(x) + bias into the interior of PCL z.
 *   epilogue 0: raw output (+ residual[v][c] if given); if stat_mean != NULL also writes
 *               BatchNorm partials: stat_mean/stat_m2 [parts][32], stat_cnt [parts] with
 *               parts = as_conv32_stat_parts() (capacity as_conv32_num_blocks() always suffices);
 *   epilogue 1: z = lrelu(acc*ep_scale[c] + ep_shift[c]) (+ residual[v][c] if given):
 *               eval-mode BatchNorm + LeakyReLU (+ BasicBlock skip) fused.
 *   z must not alias x or residual (2-D 3x3 layers with W >= 128 run on an LDS-staged kernel whose last
 *   row segment overlaps its neighbour: the overlap is computed and stored twice).  The halo of z is never
 *   written.
 * as_conv32_wgrad: dW[o][i][tap] (PyTorch layout) = sum_v x[v+tap][i] * gz[v][o];
 *   workspace must hold as_conv32_wgrad_workspace() floats. db (may be NULL) gets
 *   sum_v gz[v][o].  accumulate=1 adds into dW/db instead of overwriting them (all parameter-gradient
 *   outputs of this library have this flag: it lets a caller point them at a flat gradient arena and
 *   skip one "grad += dW" launch per parameter tensor). */
int as_conv32_pack_weights(const float* w, float* packed, const as_conv_shape* s,
                           int transpose_flip, void* stream);

/* One launch for many packings (every 32->32 convolution weight of a step, both orientations).
 * `jobs` is a DEVICE array; each job is one as_conv32_pack_weights call (taps = kd*kh*kw <= max_taps). */
typedef struct as_pack_job {
  const float* w;
  float* packed;
  int32_t taps;
  int32_t transpose_flip;   /* 0 / 1, or one of the AS_PACK_* kinds below: every weight-derived buffer of a step from ONE launch */
} as_pack_job;
#define AS_PACK_S2_DGRAD 2      /* as_conv32_dgrad_s2_pack (taps = 25) */
#define AS_PACK_CONV4 16        /* + Cin: as_conv4_pack_weights for Cin input channels (packed: taps * 128 floats) */
#define AS_PACK_MIRROR_TAP 32   /* as_mirror_taps_ch0's by_tap [9][32] of a [32][4][3][3] weight */
#define AS_PACK_MIRROR_CH 33    /* ... its by_channel [32][9] */
#define AS_PACK_WINO 34         /* as_conv32_wino_pack_weights(transposed = 0): taps = 16 (packed: 16 * 1024 floats) */
#define AS_PACK_WINO_T 35       /* ... transposed = 1: the data gradient's filter */
int as_conv32_pack_weights_batch(const as_pack_job* jobs, int njobs, int max_taps, void* stream);
int as_conv32_num_blocks(const as_pcl* gout);
int as_conv32_stat_parts(const as_pcl* gin, const as_pcl* gout, const as_conv_shape* s);
int as_conv32_fwd(const float* x, const as_pcl* gin, const float* packed_w, const float* bias,
                  float* z, const as_pcl* gout, const as_conv_shape* s,
                  int epilogue, const float* ep_scale, const float* ep_shift, float slope,
                  const float* residual, float* stat_mean, float* stat_m2, float* stat_cnt, void* stream);
/* ---- whole backward of a full-resolution refinement layer in ONE launch (csrc/conv32_bwd.hip): nn.Conv2d(32,32,3,dilation) +
 * BatchNorm2d + LeakyReLU + skip connection of a BasicBlock (stereo_net.py:10-18,33-51,97).  Replaces
 * as_conv32_wgrad_bnapply followed by as_conv32_fwd_bnbwd; g_z never leaves the chip.
 *   x, g_a, z, next_z, g_x   PCL tensors of ONE padded geometry (gin == gout; as_conv32_bwd_fused_ok() == 1)
 *   packed_wt                as_conv32_pack_weights(..., transpose_flip = 1)
 *   scale, shift, mean, coef the layer's BatchNorm state and the stage-3 coefficients [96] (as_bn_act_bwd(_given) with
 *                            g_z = NULL leaves them at workspace + as_bn_bwd_coef_offset())
 *   next_*                   the BatchNorm whose output gradient g_x is: its stage-1 sums go to next_bn_workspace
 *                            (as_bn_bwd_workspace floats; as_conv32_bwd_fused_parts() partials, for as_bn_act_bwd_given)
 *   dW [32,32,3,3], db [32]  set or accumulated; workspace: as_conv32_bwd_fused_workspace() floats */
int as_conv32_bwd_fused_ok(const as_pcl* gin, const as_pcl* gout, const as_conv_shape* s);
int as_conv32_bwd_fused_parts(void);
int64_t as_conv32_bwd_fused_workspace(void);
int as_conv32_bwd_fused(const float* x, const as_pcl* gin, const float* g_a, const float* z, const as_pcl* gout,
                        const as_conv_shape* s, const float* packed_wt, const float* scale, const float* shift,
                        const float* mean, const float* coef, float slope, const float* next_z,
                        const float* next_scale, const float* next_shift, const float* next_mean, float* g_x,
                        float* dW, float* db, int accumulate, float* next_bn_workspace, float* workspace, void* stream);

/* ---- deferred weight-gradient reductions.  Every weight-gradient entry point of the 32->32 family (as_conv32_wgrad,
 * as_conv32_wgrad_bnapply, as_conv32_bwd_fused) ends in a small reduction of per-workgroup slabs into dW / db.  Between
 * as_wgrad_defer(1) and as_wgrad_defer_flush() those reductions are only recorded and then run in ONE launch, the jobs of a
 * destination in recording order with the arithmetic of the separate launches.  The caller keeps the workspaces it passed
 * alive until the flush.  as_wgrad_defer returns the previous setting; the record is process-global (autograd runs backward
 * on its own thread). */
int as_wgrad_defer(int on);
int as_wgrad_defer_pending(void);
int as_wgrad_defer_flush(void* stream);

/* ---- training forward of a full-resolution refinement layer that forms its operand on the way in (csrc/conv32_act.hip):
 * the PREVIOUS BasicBlock's BatchNorm2d + LeakyReLU + skip connection (stereo_net.py:10-18,33-51,97) are applied to that
 * block's pre-activation while it is staged, the activated tensor is written back once as a by-product (the backward pass
 * and the next skip connection need it), and the layer's own convolution + BatchNorm moments follow.  Replaces
 * as_bn_act_fwd (previous layer) followed by as_conv32_fwd (this layer).
 *   z_prev, a_prevprev, a_out, z   PCL tensors of ONE padded geometry (gin == gout; as_conv32_act_ok() == 1)
 *   a_out = lrelu(z_prev*in_scale + in_shift) (+ a_prevprev if not NULL);  z = conv(a_out) + bias
 *   packed_w   as_conv32_pack_weights(..., transpose_flip = 0);  stat_*: (count, mean, M2) partials, as_conv32_act_parts()
 *   of them, all three or none */
int as_conv32_act_ok(const as_pcl* gin, const as_pcl* gout, const as_conv_shape* s);
int as_conv32_act_parts(void);
int as_conv32_act_fwd(const float* z_prev, const float* a_prevprev, const float* in_scale, const float* in_shift,
                      float* a_out, const as_pcl* gin, const float* packed_w, const float* bias, float slope,
                      float* z, const as_pcl* gout, const as_conv_shape* s, float* stat_mean, float* stat_m2,
                      float* stat_cnt, void* stream);

/* ---- the same layer (same arguments, same outputs) by the minimal-filtering algorithm F(2x2, 3x3) (csrc/conv32_wino.hip):
 * four 32x32 matrix products per output pixel where the direct form has nine; dilation 1, 2, 4 or 8; rows of >= 64 pixels.
 * The result differs from as_conv32_act_fwd's by fp32 rounding only (a different, equally valid association).
 *   wino_w     as_conv32_wino_pack_weights(w, out, transposed = 0) — 16 * 1024 floats — or a batch job of kind AS_PACK_WINO
 *   stat_*     as_conv32_wino_parts() partials */
int as_conv32_wino_ok(const as_pcl* gin, const as_pcl* gout, const as_conv_shape* s);
int as_conv32_wino_parts(void);
int as_conv32_wino_pack_weights(const float* w, float* packed, int transposed, void* stream);
int as_conv32_wino_fwd(const float* z_prev, const float* a_prevprev, const float* in_scale, const float* in_shift,
                       float* a_out, const as_pcl* gin, const float* wino_w, const float* bias, float slope,
                       float* z, const as_pcl* gout, const as_conv_shape* s, float* stat_mean, float* stat_m2,
                       float* stat_cnt, void* stream);

/* ---- eval-mode BasicBlock (stereo_net.py:10-18 with BatchNorm folded to an affine) by minimal filtering:
 *   out = lrelu((conv(x) + bias) * scale + shift) (+ x if residual != 0);  x, out: PCL tensors of geometry g (zero halo),
 *   as_conv32_wino_ok(g, g, s) == 1;  wino_w as for as_conv32_wino_fwd;  bias may be NULL */
int as_conv32_wino_eval(const float* x, const as_pcl* g, const as_conv_shape* s, const float* wino_w, const float* bias,
                        const float* scale, const float* shift, float slope, int residual, float* out, void* stream);

/* ---- backward of that layer by minimal filtering, two launches (csrc/conv32_wino.hip MODE 2, csrc/conv32_wino_wgrad.hip):
 * arguments and results of as_conv32_bwd_fused (below), except
 *   wino_wt    as_conv32_wino_pack_weights(w, out, transposed = 1) or a batch job of kind AS_PACK_WINO_T
 *   g_z        a PCL buffer of the layer's geometry with a zero halo: receives the gradient w.r.t. the pre-activation
 *   next_bn_workspace   as_conv32_wino_bwd_parts() partials of [64] doubles;  workspace: as_conv32_wino_bwd_workspace() floats */
int as_conv32_wino_bwd_parts(void);
int64_t as_conv32_wino_bwd_workspace(void);
/* which data-gradient kernel as_conv32_wino_bwd_data launches: 2 (default) = csrc/conv32_wino_dgrad.hip — the waves of a
 * workgroup have roles, the skip connection's g_a rows stay in LDS between conversion and output (one HBM read of g_a instead
 * of two), rows are staged 64 + 2 * dilation voxels wide — for dilation 1, 2, 4 and csrc/conv32_wino.hip MODE 2 for dilation 8
 * (where the second generation's LDS ring does not fit and it is the slower one); 1 = csrc/conv32_wino.hip MODE 2 always;
 * 3 = csrc/conv32_wino_dgrad.hip always (parity tests).  Same bits in every case (what the parity tests hold them to);
 * returns the previous setting, any other argument only queries */
int as_conv32_wino_bwd_generation(int generation);
/* the two launches separately (the weight gradient may go to another stream: only the step's slab reduction waits for it) */
int as_conv32_wino_bwd_data(const float* g_a, const float* z, const as_pcl* g, const as_conv_shape* s,
                            const float* wino_wt, const float* scale, const float* shift, const float* mean,
                            const float* coef, float slope, const float* next_z, const float* next_scale,
                            const float* next_shift, const float* next_mean, float* g_z, float* g_x,
                            float* next_bn_workspace, void* stream);
int as_conv32_wino_bwd_filter(const float* x, const float* g_z, const as_pcl* g, const as_conv_shape* s, float* dW,
                              float* db, int accumulate, float* workspace, void* stream);
int as_conv32_wino_bwd(const float* x, const as_pcl* gin, const float* g_a, const float* z, const as_pcl* gout,
                       const as_conv_shape* s, const float* wino_wt, const float* scale, const float* shift,
                       const float* mean, const float* coef, float slope, const float* next_z,
                       const float* next_scale, const float* next_shift, const float* next_mean, float* g_z,
                       float* g_x, float* dW, float* db, int accumulate, float* next_bn_workspace,
                       float* workspace, void* stream);
/* ---- the same backward in ONE launch (csrc/conv32_wino_bwd.hip): one 8-wave workgroup per CU, waves 0-3 the data gradient,
 * waves 4-7 the weight gradient on the g_z rows the first four keep in LDS — g_z never goes to HBM (x, g_a, z, next_z read, g_x
 * written: 5 tensor passes for the two launches' 7).  Arguments of as_conv32_wino_bwd without g_z; g_x equals the two-launch
 * result bit for bit, dW / db to rounding (another order of the sum over tiles).
 *   next_bn_workspace   as_conv32_wino_bwd_fused_parts() partials of [64] doubles;  workspace: as_conv32_wino_bwd_fused_workspace() floats
 * Replaces, per layer of EdgeAwareRefinement (reference models/stereo_net.py:10-18, 33-51, 97), autograd's conv2d backward +
 * BatchNorm backward + LeakyReLU backward + the residual add. */
int as_conv32_wino_bwd_fused_parts(void);
int64_t as_conv32_wino_bwd_fused_workspace(void);
int as_conv32_wino_bwd_fused(const float* x, const as_pcl* gin, const float* g_a, const float* z, const as_pcl* gout,
                             const as_conv_shape* s, const float* wino_wt, const float* scale, const float* shift,
                             const float* mean, const float* coef, float slope, const float* next_z,
                             const float* next_scale, const float* next_shift, const float* next_mean, float* g_x,
                             float* dW, float* db, int accumulate, float* next_bn_workspace, float* workspace, void* stream);

/* ---- the 5x5 stride-2 32->32 layers of the feature head (stereo_net.py:59-72): as_conv32_fwd and as_conv32_dgrad_s2(_packed)
 * run them on csrc/conv32_s2.hip (coalesced row staging through wave-private LDS) when the map fills the chip; 0 switches back to
 * the generic direct-load kernels (same bits: the parity tests compare them).  Returns the previous setting; any other argument
 * only queries */
int as_conv32_s2_enable(int on);
/* the same switch for the towers' FIRST layer, nn.Conv2d(3, 32, 5, stride=2, padding=2) (stereo_net.py:61-69): as_conv4_fwd runs
 * it on conv4_s2_fwd_kernel (persistent waves, rows staged through wave-private LDS) when the epilogue is plain and the map fills
 * the chip; bit-identical to conv4_fwd_kernel<25> */
int as_conv4_s2_enable(int on);
/* Read-only route queries: what the entry points would launch NOW for this geometry, switch included (the routes give equal bits
 * by design, so only a query can tell a test which kernel ran).  1 / 0, or AS_ERR_ARG where the entry point would refuse.
 *   as_conv4_s2_ok          as_conv4_fwd with a plain epilogue (0) and no moments launches conv4_s2_fwd_kernel
 *   as_conv32_s2_fwd_ok     as_conv32_fwd with epilogue 0, no residual and no moments launches conv32_s2_fwd_kernel (switch on,
 *                           the map fills the chip, and split-K does not take precedence)
 *   as_conv32_s2_dgrad_ok   as_conv32_dgrad_s2_packed launches conv32_s2_dgrad_kernel
 *   as_conv32_wgrad_segments  segments per row of as_conv32_wgrad's generic kernel (>= 1), 0 when an LDS kernel takes the layer */
int as_conv4_s2_ok(const as_pcl* gin, const as_pcl* gout, const as_conv_shape* s);
int as_conv32_s2_fwd_ok(const as_pcl* gin, const as_pcl* gout, const as_conv_shape* s);
int as_conv32_s2_dgrad_ok(const as_pcl* ggz, const as_pcl* ggx);
int as_conv32_wgrad_segments(const as_pcl* gin, const as_pcl* gout, const as_conv_shape* s);

/* ---- the refinement's output layer with the last BasicBlock's activation on the way in (csrc/refine_out.hip;
 * stereo_net.py:44-51, 102, 116-121):  out = relu?(conv2d_out(a) + bias + add_src)  where
 *   scale != NULL:  a = lrelu(x * scale + shift) (+ skip) — x is the block's pre-activation, scale / shift its BatchNorm as an
 *                   affine; a is also written to a_out (the backward pass and nothing else reads it)
 *   scale == NULL:  a = x (already activated: inference); skip, shift, a_out must be NULL
 *   x, skip, a_out  PCL tensors of geometry g (as_refine_out_ok(g) == 1: 2-D, halo >= 1);  w [32][9], bias [1] or NULL
 *   add_src, out    dense [B][H][W] */
int as_refine_out_ok(const as_pcl* g);
int as_refine_out_fwd(const float* x, const float* skip, const float* scale, const float* shift, float slope, float* a_out,
                      const as_pcl* g, const float* w, const float* bias, const float* add_src, int relu, float* out,
                      void* stream);

/* ---- a3, second generation: one 3x3x3 stride-1 32->32 aggregation layer (stereo_net.py:21-30,155-161,185-186) or its data
 * gradient, walking down the disparity axis with a rolling window of planes in LDS (csrc/agg3d.hip).
 *   x, z, a_out      PCL tensors of geometry g (halo 1 in d, h, w; as_agg3d_ok(g) == 1)
 *   in_scale/shift   non-null: x is the PREVIOUS layer's raw convolution output and lrelu(x*in_scale + in_shift) — that
 *                    layer's BatchNorm + LeakyReLU(slope) — is applied on the fly; a_out (optional) receives the activated
 *                    tensor (what nn.Sequential would have materialised: the backward pass needs it)
 *   in_bn            alternative to in_scale/shift: the previous layer's BatchNorm is still in PARTIALS (what its own launch
 *                    wrote through stat_*): every workgroup merges them (as_bn_finalize's arithmetic) while its first planes
 *                    are in flight, workgroup 0 writes that layer's state and running statistics — no finalize launch
 *   epilogue         0: z = conv + bias, and (count, mean, M2) BatchNorm partials if stat_* are given (as_agg3d_parts(g)
 *                    partials); 1: z = lrelu((conv + bias)*ep_scale + ep_shift) (eval mode); 2: as 0 without moments */
typedef struct as_bn_merge {
  const float* stat_mean;   /* [nparts][32] */
  const float* stat_m2;     /* [nparts][32] */
  const float* stat_cnt;    /* [nparts] */
  const float* gamma;
  const float* beta;
  float* running_mean;      /* may be NULL (with running_var) */
  float* running_var;
  float* save_mean;         /* outputs, [32] each */
  float* save_invstd;
  float* scale;
  float* shift;
  int32_t nparts;
  float momentum;
  float eps;
} as_bn_merge;
int as_agg3d_ok(const as_pcl* g);
int as_agg3d_parts(const as_pcl* g);
/* read-only plan query, from the helper the launcher fills its argument block with: out = {strips, Ws (row pitch of the staged
 * (sub-)plane), tiles per strip, npos (positions of a (sub-)plane from its first to its last interior voxel), run (staged voxels
 * per plane), seg_len (output planes per unit), nseg, units}; the grid is 8 * ceil(units / 8) workgroups.  Returns 1, or 0
 * where as_agg3d_ok(g) == 0 (out untouched).  Every plan gives equal outputs by design: only the query tells which one ran. */
int as_agg3d_plan(const as_pcl* g, int out[8]);
int as_agg3d_fwd(const float* x, const as_pcl* g, const float* packed_w, const float* bias,
                 const float* in_scale, const float* in_shift, const as_bn_merge* in_bn, float* a_out,
                 float* z, int epilogue, const float* ep_scale, const float* ep_shift, float slope,
                 float* stat_mean, float* stat_m2, float* stat_cnt, void* stream);

/* ---- a4 + a5 + a8 in one launch: conv3d_alone (stereo_net.py:162,187) -> logits -> soft-argmax (:190-192,124-134),
 * arg-max index and feature-contrast score (utils/feature_contrast.py:12-23), csrc/agg_tail.hip.
 *   x                PCL volume of geometry g (halo 1; as_agg_tail_ok(g) == 1): the last aggregation layer's ACTIVATED output,
 *                    or — with in_scale/in_shift — its RAW convolution output, whose BatchNorm + LeakyReLU(slope) is then
 *                    applied on the fly (a_out, optional, receives the activated tensor for the backward pass); in_bn: as for
 *                    as_agg3d_fwd (the layer's BatchNorm still in partials, merged by every workgroup)
 *   w, bias          conv3d_alone.weight [1,32,3,3,3] (PyTorch order) and bias [1] (may be NULL)
 *   logits           dense [B,D,H,W];  pred, fcs: dense float [B,H,W];  argmax: int32 [B,H,W] (first maximum, as torch.argmax);
 *                    argmax and fcs may be NULL */
int as_agg_tail_ok(const as_pcl* g);
/* read-only route query: positions of the flattened padded plane per workgroup that as_agg_tail_fwd launches with for this
 * geometry, 16 (agg_tail_direct_kernel<.., 16>: B * ceil(npos / 32) < 512, npos = (H - 1)(W + 2) + W) or 32; 0 where
 * as_agg_tail_ok(g) == 0.  The two give equal logits by design: only the query tells which kernel ran. */
int as_agg_tail_fwd_positions(const as_pcl* g);
int as_agg_tail_fwd(const float* x, const as_pcl* g, const float* in_scale, const float* in_shift,
                    const as_bn_merge* in_bn, float* a_out,
                    const float* w, const float* bias, float slope, float* logits, float* pred,
                    int32_t* argmax, float* fcs, void* stream);

/* ---- a1, the 1/2^k-resolution trunk of FeatureExtractorNetwork in train mode (csrc/trunk.hip): six BasicBlocks
 * a_l = lrelu(BN_l(conv3x3_l(a_{l-1}))) + a_{l-1} (stereo_net.py:33-51, only conv1 is executed) and conv_alone (:85), called
 * once per image of a pair (adapt.py:72) — here ONE launch per layer and direction for both images: the batch dimension of
 * every PCL tensor holds `ngroups` statistics groups of B/ngroups images each (left images, then right images), BatchNorm
 * moments and gradients are taken per group, as the two separate calls of the reference take them.
 * Replaces, per BasicBlock and image: as_conv32_fwd + as_bn_finalize + as_bn_act_fwd forward and as_bn_act_bwd (three kernels) +
 * as_conv32_wgrad + as_conv32_fwd(dgrad) backward.
 *   geometry g       2-D PCL (D = 1, halo >= 1 in h and w), any H, W
 *   as_trunk_parts   workgroups per group of a launch = BatchNorm partials per group = weight-gradient slabs / ngroups
 * as_trunk_fwd: z = conv3x3(operand) + bias and, if stat_* are given, per-workgroup (count, mean, M2) moments of z
 *   [ngroups * parts] (+[32]).  bn_prev == NULL: the operand is `src`.  bn_prev != NULL: the operand is
 *   a_prev = lrelu(BN_prev(src)) + skip with BN_prev still in the partials its own launch wrote; every workgroup merges its
 *   group's partials (as_bn_finalize's arithmetic, fp64), the first workgroup of a group writes
 *   state[group] = {mean, invstd, scale, shift, unbiased variance}[32], and a_prev is written to a_out.
 * as_trunk_finish_fwd: features PCL -> NCHW, and running_mean/var of `nlayers` BatchNorm layers updated from `states`
 *   ([nlayers][ngroups][5][32]) group after group (feature_net(left), then feature_net(right)); running_mean / running_var are
 *   HOST arrays of nlayers device pointers.
 * as_trunk_bwd: backward of one layer.  z != NULL (a BasicBlock): g_a = dL/da_l; g_z = BatchNorm-backward(lrelu'(.) g_a) with
 *   the per-group sums merged from `sums` ([ngroups][nparts][64] doubles: what the launch above it left in sums_next);
 *   bn_grads [ngroups][2][32] receives the group's (g_gamma, g_beta); g_x = g_a + dgrad(g_z).  z == NULL (conv_alone): g_a is
 *   the gradient of the convolution's output itself, g_x = dgrad(g_a).  Both: dW [32,32,3,3] / db [32] set or accumulated
 *   (workspace: as_trunk_bwd_workspace floats, kept alive until as_wgrad_defer_flush inside a deferral region), and, if z_next is
 *   given, the stage-1 sums of the layer below (its pre-activation z_next, its state) into sums_next
 *   ([ngroups * parts][64] doubles).
 * as_trunk_finish_bwd: g_gamma[l] / g_beta[l] (HOST arrays of device pointers) set or accumulated from bn_grads
 *   ([nlayers][ngroups][2][32]), groups in call order. */
typedef struct as_trunk_bn {
  const float* stat_mean;   /* [ngroups][nparts][32] */
  const float* stat_m2;     /* [ngroups][nparts][32] */
  const float* stat_cnt;    /* [ngroups][nparts] */
  const float* gamma;
  const float* beta;
  float* state;             /* out: [ngroups][5][32] */
  int32_t nparts;           /* partials per group */
  float eps;
} as_trunk_bn;
int as_trunk_parts(const as_pcl* g, int ngroups);
int as_trunk_fwd(const float* src, const float* skip, const as_trunk_bn* bn_prev, float* a_out, const as_pcl* g, int ngroups,
                 const float* packed_w, const float* bias, float slope, float* z, float* stat_mean, float* stat_m2,
                 float* stat_cnt, void* stream);
int as_trunk_finish_fwd(const float* feats_pcl, const as_pcl* g, float* feats_nchw, const float* states, int nlayers,
                        int ngroups, float* const* running_mean, float* const* running_var, float momentum, void* stream);
 /* as_trunk_begin_bwd: the features' gradient(s), NCHW — one tensor [B,32,H,W] (g_b NULL, nA = B) or the left and right
 * halves of a pair pass separately ([nA,...] and [B-nA,...]) — into the interior of one PCL buffer of geometry g. */
int as_trunk_begin_bwd(const float* g_a, const float* g_b, int nA, const as_pcl* g, float* out_pcl, void* stream);
int64_t as_trunk_bwd_workspace(const as_pcl* g, int ngroups);
int as_trunk_bwd(const float* g_a, const float* z, const float* state, const double* sums, int nparts, const float* gamma,
                 float* bn_grads, const float* x, const float* packed_wt, float* g_x, const float* z_next,
                 const float* state_next, double* sums_next, const as_pcl* g, int ngroups, float slope, float* dW, float* db,
                 int accumulate, float* workspace, void* stream);
int as_trunk_finish_bwd(const float* bn_grads, int nlayers, int ngroups, float* const* g_gamma, float* const* g_beta,
                        int accumulate, void* stream);

/* Data gradient of nn.Conv2d(32,32,5,stride=2,padding=2) (FeatureExtractorNetwork.downsample[1..k-1],
 * stereo_net.py:61-69): four parity phases of a transposed convolution, each a gather over gz.
 * gz: PCL of the convolution's output extent (halo >= 1); gx: PCL of its input extent; w: PyTorch
 * [32][32][5][5]; workspace: as_conv32_dgrad_s2_workspace() floats. */
int64_t as_conv32_dgrad_s2_workspace(void);
int as_conv32_dgrad_s2(const float* gz, const as_pcl* ggz, const float* w, float* gx, const as_pcl* ggx,
                       float* workspace, void* stream);
/* The same in two halves: the phase-major packing of the weights (25 * 1024 floats; constant while the weights are) and the
 * convolution on packed weights — a caller that packs once per step (or through as_conv32_pack_weights_batch, AS_PACK_S2_DGRAD)
 * saves the packing launch of every call. */
int as_conv32_dgrad_s2_pack(const float* w, float* packed, void* stream);
int as_conv32_dgrad_s2_packed(const float* gz, const as_pcl* ggz, const float* packed, float* gx, const as_pcl* ggx,
                              void* stream);
int64_t as_conv32_wgrad_workspace(const as_pcl* gin, const as_pcl* gout, const as_conv_shape* s);
int as_conv32_wgrad(const float* x, const as_pcl* gin, const float* gz, const as_pcl* gout,
                    const as_conv_shape* s, float* dW, float* db, int accumulate, float* workspace, void* stream);
/* Host-side view of the work assignment of the LDS-staged 3-D weight gradient (csrc/conv3d_lds.hip): chunk, kd and extra tile
 * (-1: none) of workgroup `block` for a launch over ntiles tiles in nchunks chunks; returns 1 (working block) / 0 (padding
 * block).  Runs on the host — the function the kernel itself calls — so that a test without a GPU can check that every
 * tile is covered exactly three times for any (ntiles, nchunks). */
int as_conv3d_wgrad_lds_assignment(int ntiles, int nchunks, int block, int* chunk, int* kd, int* extra_tile);

/* ---- BatchNorm (train/eval) + LeakyReLU around the convolution --------------
 * nn.BatchNorm3d / nn.BatchNorm2d (eps, momentum as given) + nn.LeakyReLU(0.2)
 * (stereo_net.py:17,29,39,94,159).
 * as_bn_finalize: merges the conv's (count, mean, M2) partials (Chan, fp64),
 *   writes save_mean/save_invstd, scale = gamma*invstd, shift = beta - mean*scale,
 *   and updates running_mean / running_var (unbiased) with `momentum`.
 * as_bn_eval_affine: scale/shift from the running statistics (eval mode).
 * as_bn_act_fwd: a = lrelu(z*scale+shift) (+ residual) on the interior.
 * as_bn_act_bwd: given g_a, z: writes g_z (PCL interior), g_gamma, g_beta; train=1 uses
 *   batch statistics (full BatchNorm backward), train=0 treats mean/invstd as constants.
 *   workspace: as_bn_bwd_workspace() floats. If g_res != NULL it receives nothing (the
 *   skip connection's gradient is g_a itself and is handled by the caller). */
int as_bn_finalize(const float* stat_mean, const float* stat_m2, const float* stat_cnt, int nparts,
                   const float* gamma, const float* beta, float* running_mean, float* running_var,
                   float momentum, float eps, float* save_mean, float* save_invstd,
                   float* scale, float* shift, void* stream);
int as_bn_eval_affine(const float* gamma, const float* beta, const float* running_mean,
                      const float* running_var, float eps, float* save_mean, float* save_invstd,
                      float* scale, float* shift, void* stream);
/* as_bn_eval_affine for many layers in one launch; `jobs` is a DEVICE array, out = [mean, invstd, scale, shift][32]. */
typedef struct as_bn_affine_job {
  const float* gamma;
  const float* beta;
  const float* running_mean;
  const float* running_var;
  float* out;
} as_bn_affine_job;
int as_bn_eval_affine_batch(const as_bn_affine_job* jobs, int njobs, float eps, void* stream);
int as_bn_act_fwd(const float* z, const float* scale, const float* shift, float slope,
                  const float* residual, float* a, const as_pcl* g, void* stream);
int64_t as_bn_bwd_workspace(const as_pcl* g);
int as_bn_act_bwd(const float* g_a, const float* z, const float* scale, const float* shift,
                  const float* save_mean, const float* save_invstd, const float* gamma,
                  float slope, int train, float* g_z, float* g_gamma, float* g_beta, int accumulate,
                  float* workspace, const as_pcl* g, void* stream);
/* Data gradient of a convolution fused with stage 1 (the per-channel sums) of the BatchNorm backward that consumes
 * its output: z_out = conv(x) (+ residual) IS the g_a of the layer whose pre-activation is bn_z, so
 * sum g_y and sum g_y*(bn_z - mean), g_y = z_out * lrelu'(bn_z*scale + shift), are taken from the output tile in
 * registers and written to bn_workspace (an as_bn_bwd_workspace() buffer) as as_conv32_bnbwd_parts() slabs;
 * as_bn_act_bwd_given then runs stages 2 and 3 only.  as_conv32_bnbwd_parts() == 0: not available for the
 * configuration (use as_conv32_fwd + as_bn_act_bwd). */
int as_conv32_bnbwd_parts(const as_pcl* gin, const as_pcl* gout, const as_conv_shape* s);
int as_conv32_fwd_bnbwd(const float* x, const as_pcl* gin, const float* packed_w, float* z_out, const as_pcl* gout,
                        const as_conv_shape* s, const float* residual, const float* bn_z,
                        const float* bn_scale, const float* bn_shift, const float* bn_mean, float slope,
                        float* bn_workspace, void* stream);
/* Stage 3 (g_z = (g_a*lrelu'(z*scale+shift) - k1 - (z-mean)*k2)*k3) fused into the weight gradient of the same layer:
 * call as_bn_act_bwd / as_bn_act_bwd_given with g_z = NULL (stages 1-2 only; the coefficients k1,k2,k3 stay in the
 * workspace at float offset as_bn_bwd_coef_offset()), then as_conv32_wgrad_bnapply, which stages g_a and z rows, applies
 * stage 3 in LDS, accumulates dW/db from the result and writes g_z (PCL interior) for the data gradient that follows.
 * Available when as_conv32_wgrad_bnapply_ok() == 1 (launches that fill the chip). */
int64_t as_bn_bwd_coef_offset(void);
int as_conv32_wgrad_bnapply_ok(const as_pcl* gin, const as_pcl* gout, const as_conv_shape* s);
int as_conv32_wgrad_bnapply(const float* x, const as_pcl* gin, const float* g_a, const float* z, const as_pcl* gout,
                            const as_conv_shape* s, const float* scale, const float* shift, const float* mean,
                            const float* coef, float slope, float* g_z, float* dW, float* db, int accumulate,
                            float* workspace, void* stream);
int as_bn_act_bwd_given(const float* g_a, const float* z, const float* scale, const float* shift,
                        const float* save_mean, const float* save_invstd, const float* gamma,
                        float slope, int train, float* g_z, float* g_gamma, float* g_beta, int accumulate,
                        float* workspace, const as_pcl* g, int nparts, void* stream);

/* Cross-replica ("synchronised") BatchNorm in data-parallel adaptation (the reference's train-mode
 * BatchNorm, stereo_net.py:17,29, sees the whole batch).  Forward needs nothing new: the replicas exchange their
 * convolution partials (count, mean, M2) and every one calls as_bn_finalize on the concatenation.  Backward splits
 * as_bn_act_bwd at the point where the replicas must meet:
 *   as_bn_bwd_sums: stage 1 (skipped when nparts_given > 0: the slabs are already in the workspace, see
 *     as_conv32_fwd_bnbwd) + the fixed-order slab sum -> sums[65] doubles = [sum g_y][32], [sum g_y*(z-mean)][32],
 *     element count.  The caller all-reduces (sum) a COPY of it.
 *   as_bn_bwd_finalize_synced: g_gamma / g_beta from this replica's sums (the parameter-gradient all-reduce adds the
 *     replicas' later), stage-3 coefficients from the all-reduced sums and count, left in the workspace at
 *     as_bn_bwd_coef_offset().
 *   as_bn_bwd_apply: stage 3 alone (g_z on the PCL interior); as_conv32_wgrad_bnapply / as_conv4_wgrad_bnapply take the
 *     same coefficients instead when stage 3 rides on the weight gradient. */
int as_bn_bwd_sums(const float* g_a, const float* z, const float* scale, const float* shift,
                   const float* save_mean, float slope, float* workspace, const as_pcl* g,
                   int nparts_given, double* sums, void* stream);
int as_bn_bwd_finalize_synced(const double* local_sums, const double* global_sums, const float* save_invstd,
                              const float* gamma, float* g_gamma, float* g_beta, int accumulate,
                              float* workspace, void* stream);
int as_bn_bwd_apply(const float* g_a, const float* z, const float* scale, const float* shift,
                    const float* save_mean, float slope, float* g_z, const float* workspace,
                    const as_pcl* g, void* stream);

/* ---- a4 + a5 + a8: conv3d 32->1, soft-argmax, arg-max index, FCS ---------------
 * nn.Conv3d(32,1,3,padding=1) (stereo_net.py:162,187), F.softmax(dim=1) +
 * DisparityRegression (stereo_net.py:190-192,124-134), feature_contrast_mean
 * (utils/feature_contrast.py:12-23).
 * w: [32][27] (PyTorch [1][32][3][3][3]).  logits: [B][D][H][W] (the reference's
 * "cost_volume_{side}/{scale}" output).  pred/fcs: [B][H][W]; argmax: int32 [B][H][W]. */
int as_conv3d_out_fwd(const float* a, const as_pcl* g, const float* w, const float* bias,
                      float* logits, void* stream);
int64_t as_conv3d_out_bwd_workspace(const as_pcl* g);
int as_conv3d_out_bwd(const float* g_logits, const float* a, const as_pcl* g, const float* w,
                      float* g_a, float* g_w, float* g_bias, int accumulate, float* workspace, void* stream);
int as_softargmax_fwd(const float* logits, int B, int D, int H, int W,
                      float* pred, int32_t* argmax, float* fcs, void* stream);
/* g_logits[d] = p_d*(d - pred)*g_pred (+ g_logits_in[d] when not NULL). */
int as_softargmax_bwd(const float* logits, const float* g_pred, const float* g_logits_in,
                      int B, int D, int H, int W, float* g_logits, void* stream);

/* The backward of a5 + a4 in ONE launch (csrc/agg_tail_bwd.hip): the logits gradient p_d*(d - pred)*g_pred (+ g_logits_in) is
 * formed in LDS per (row, 4 disparity planes) and feeds the data gradient g_a and the weight / bias gradient of conv3d_alone from
 * one read of the activation a; it never reaches HBM.  g_pred [B][H][W], g_logits_in [B][D][H][W]: either may be NULL (zero).
 * a, g_a: PCL of geometry g; g_w [32][27], g_bias [1] (may be NULL): overwritten, or added to with accumulate != 0.
 * workspace: as_agg_tail_bwd_workspace(g) floats.  as_agg_tail_bwd_ok(g) == 0: use as_softargmax_bwd + as_conv3d_out_bwd. */
int as_agg_tail_bwd_ok(const as_pcl* g);
int64_t as_agg_tail_bwd_workspace(const as_pcl* g);
/* read-only route query: columns per unit that as_agg_tail_bwd launches with for this geometry, 13 (agg_tail_bwd_kernel<13>:
 * B * H * ceil(W / 26) <= 768) or 26; 0 where as_agg_tail_bwd_ok(g) == 0 */
int as_agg_tail_bwd_columns(const as_pcl* g);
int as_agg_tail_bwd(const float* logits, const float* g_pred, const float* g_logits_in, const float* a, const as_pcl* g,
                    const float* w, float* g_a, float* g_w, float* g_bias, int accumulate, float* workspace, void* stream);

/* ---- generic 32 -> 1 convolution (3x3x3 or 3x3, 'same' padding, any dilation) ----------
 * The 3-D instance is a4 above; the 2-D instance is EdgeAwareRefinement.conv2d_out =
 * nn.Conv2d(32,1,3,padding=1) with the block's tail fused: out = relu(add_src + conv(a) + bias)
 * (stereo_net.py:102,121).  It also serves as the data-gradient of conv2d_feature w.r.t. its
 * disparity channel (a 32->1 convolution with mirrored taps).  w: [32][taps]; out/add_src/g_out:
 * dense [B][D][H][W].  bwd: g_a (PCL, may be NULL), g_w [32][taps] (may be NULL), g_bias [1] (may be NULL). */
int as_conv32to1_fwd(const float* a, const as_pcl* g, const as_conv_shape* s, const float* w,
                     const float* bias, const float* add_src, int relu, float* out, void* stream);
int64_t as_conv32to1_bwd_workspace(const as_pcl* g, const as_conv_shape* s);
int as_conv32to1_bwd(const float* g_out, const float* a, const as_pcl* g, const as_conv_shape* s,
                     const float* w, float* g_a, float* g_w, float* g_bias, int accumulate, float* workspace,
                     void* stream);
/* Data gradient of the 2-D 3x3 32->1 output layer (conv2d_out, stereo_net.py:102) that also produces stage 1 of the
 * BatchNorm backward consuming it — per-channel sums of g_a*lrelu'(z*scale+shift) and of that times (z - mean) — as
 * as_conv32to1_bnsums_parts(g) fp64 slabs in bn_workspace (as_bn_bwd_workspace floats), for as_bn_act_bwd_given.
 * Replaces as_conv32to1_bwd(g_a only) + the as_bn_bwd_sums pass over g_a and z. */
int as_conv32to1_bnsums_ok(const as_pcl* g, const as_conv_shape* s);
int as_conv32to1_bnsums_parts(const as_pcl* g);
int as_conv32to1_dgrad_bnsums(const float* g_out, const as_pcl* g, const as_conv_shape* s, const float* w, float* g_a,
                              const float* bn_z, const float* bn_scale, const float* bn_shift, const float* bn_mean,
                              float slope, float* bn_workspace, void* stream);

/* ---- thin-input convolution: Cin <= 4 -> 32 on "PCL4" ([B][H+2ph][W+2pw][4], zero halo) -----
 * EdgeAwareRefinement.conv2d_feature = nn.Conv2d(4,32,3,padding=1) over cat([disparity, rgb])
 * (stereo_net.py:89-94,116-118) and FeatureExtractorNetwork.downsample[0] = nn.Conv2d(3,32,5,
 * stride=2,padding=2) (:61-69).  as_pack_in4 builds the PCL4 image from an optional dense plane
 * ch0 [B,1,H,W] followed by the C channels of img [B,C,H,W] (this is the reference's torch.cat).
 * Epilogue arguments as for as_conv32_fwd.  wgrad: dW in PyTorch layout [32][Cin][kh][kw]. */
int64_t as_pcl4_numel(const as_pcl* g);
int as_pack_in4(const float* ch0, const float* img, int C, float* x4, const as_pcl* g, void* stream);
int as_conv4_pack_weights(const float* w, int Cin, float* packed, const as_conv_shape* s, void* stream);
/* Number of (mean, M2, count) partials as_conv4_fwd writes for this configuration (size of stat_*). */
int as_conv4_stat_parts(const as_pcl* gin, const as_pcl* gout, const as_conv_shape* s);
int as_conv4_fwd(const float* x4, const as_pcl* gin, const float* packed_w, const float* bias,
                 float* z, const as_pcl* gout, const as_conv_shape* s,
                 int epilogue, const float* ep_scale, const float* ep_shift, float slope,
                 float* stat_mean, float* stat_m2, float* stat_cnt, void* stream);
/* as_conv4_wgrad with stage 3 of the layer's BatchNorm backward applied on the fly (gradient operand = g_a, g_z written as
 * a by-product; coefficients from as_bn_act_bwd(g_z = NULL), see as_conv32_wgrad_bnapply).  3x3 stride-1 layers only. */
int as_conv4_wgrad_bnapply_ok(const as_pcl* gin, const as_pcl* gout, const as_conv_shape* s);
int as_conv4_wgrad_bnapply(const float* x4, const as_pcl* gin, const float* g_a, const float* z, const as_pcl* gout,
                           const as_conv_shape* s, int Cin, const float* scale, const float* shift, const float* mean,
                           const float* coef, float slope, float* g_z, float* dW, float* db, int accumulate,
                           float* workspace, void* stream);
/* as_conv4_wgrad_bnapply without the g_z write: what goes out are the nine per-tap projections
 * h[b][t][y][x] = sum_co g_z[b][y][x][co] * w_proj[t][co]  (t = 3*kh + kw, w_proj [9][32]) — all that the 3x3 32->1 data
 * gradient of conv2d_feature's disparity channel (stereo_net.py:116-118) needs; as_tap_gather then forms
 * out[b][y][x] = residual[b][y][x] + sum_t h[b][t][y + kh - 1][x + kw - 1] (zero outside the image; residual may be NULL). */
int as_conv4_wgrad_bnapply_proj(const float* x4, const as_pcl* gin, const float* g_a, const float* z, const as_pcl* gout,
                                const as_conv_shape* s, int Cin, const float* scale, const float* shift, const float* mean,
                                const float* coef, float slope, const float* w_proj, float* h, float* dW, float* db,
                                int accumulate, float* workspace, void* stream);
int as_tap_gather(const float* h, const float* residual, float* out, int B, int H, int W, void* stream);
int64_t as_conv4_wgrad_workspace(const as_pcl* gout, const as_conv_shape* s);
int as_conv4_wgrad(const float* x4, const as_pcl* gin, const float* gz, const as_pcl* gout,
                   const as_conv_shape* s, int Cin, float* dW, float* db, int accumulate, float* workspace,
                   void* stream);

/* ---- a6/a7 head: bilinear up-sampling, align_corners=False -------------------
 * F.interpolate(pred.unsqueeze(1), size=(H,W), mode="bilinear") * gain
 * (stereo_net.py:106-114, 201-202).  src: [B][h][w], dst: [B][1][H][W]. */
int as_upsample_bilinear_fwd(const float* src, int B, int h, int w, float* dst, int H, int W,
                             float gain, void* stream);
int as_upsample_bilinear_bwd(const float* g_dst, int B, int H, int W, float* g_src, int h, int w,
                             float gain, void* stream);

/* ---- a9: LinearWarping — models/linear_warping.py:18-57 -----------------------
 * grid_sample(bilinear, border, align_corners=False) at (x -/+ disp, y) after the
 * 2x/w-1 normalisation => samples at (x -/+ d - 0.5, y - 0.5).  img: NCHW [B,C,H,W];
 * disp: [B,1,H,W]; warped: [B,C,H,W]; mask: uint8 [B,1,H,W].  bwd: gradient w.r.t.
 * disp only (the image has no gradient in the adaptation loss). */
int as_warp_fwd(const float* img, const float* disp, int B, int C, int H, int W, int right_to_left,
                float* warped, uint8_t* mask, void* stream);
int as_warp_bwd(const float* g_warped, const float* img, const float* disp, int B, int C, int H, int W,
                int right_to_left, float* g_disp, void* stream);
/* LinearWarping.forward(mode="nearest") (models/linear_warping.py:57 forwards `mode` to F.grid_sample): the nearest tap of the
 * clipped sample position, ties to even; same validity mask.  No gradient w.r.t. the disparity exists in this mode. */
int as_warp_nearest_fwd(const float* img, const float* disp, int B, int C, int H, int W, int right_to_left,
                        float* warped, uint8_t* mask, void* stream);
/* The same with g_disp = (gradient through the warp) + add_src[i] (add_src may be NULL): the disparity receives its gradient
 * from the loss map directly and through the warped image (adapt.py:78-86) — the sum autograd would form in a launch of its own. */
int as_warp_bwd_add(const float* g_warped, const float* img, const float* disp, const float* add_src, int B, int C,
                    int H, int W, int right_to_left, float* g_disp, void* stream);

/* ---- a10: monodepth photometric loss — utils/loss_functions.py:41-138 ---------
 * total = 0.85*mean_c(SSIM dist) + 0.15*mean_c|I - I~| + sw*smooth(d/(mean d + 1e-7), I).
 * pred: [B,1,H,W]; img, warped: [B,3,H,W]; the four outputs: [B,1,H,W].
 * workspace: as_monodepth_workspace() floats.
 * bwd: g_* may be NULL (treated as zero).  Writes g_pred [B,1,H,W], g_warped [B,3,H,W]. */
int64_t as_monodepth_workspace(int B, int H, int W);
int as_monodepth_loss_fwd(const float* pred, const float* img, const float* warped, int B, int H, int W,
                          float smoothness_weight, float* total, float* l1, float* ssim, float* smooth,
                          float* workspace, void* stream);
int as_monodepth_loss_bwd(const float* g_total, const float* g_l1, const float* g_ssim, const float* g_smooth,
                          const float* pred, const float* img, const float* warped, int B, int H, int W,
                          float smoothness_weight, float* g_pred, float* g_warped,
                          float* workspace, void* stream);
/* Backward of loss = total[mask].mean() / total[mask].sum() (adapt.py:81-83) without a dense gradient map: every valid pixel
 * of `total` carries g_sum[0] + g_mean[0] / sum_count[1] (either pointer may be NULL; sum_count = as_masked_sum's out2 of the
 * forward pass), every other pixel 0; the l1 / ssim / smooth maps carry no gradient.  fwd_workspace (may be NULL): the workspace
 * as_monodepth_loss_fwd ran with on the same pred — its per-image mean disparity is reused instead of being summed again. */
int as_monodepth_loss_bwd_masked(const uint8_t* mask, const float* g_sum, const float* g_mean, const float* sum_count,
                                 const float* pred, const float* img, const float* warped, int B, int H, int W,
                                 float smoothness_weight, float* g_pred, float* g_warped, float* workspace,
                                 const float* fwd_workspace, void* stream);

/* ---- a9 + a10 + adapt.py:81-83 in one pass each way (csrc/photometric_rows.hip) -----------------------------------------
 * monodepth_single_loss (adapt.py:78-86): warp the right image with the predicted disparity (models/linear_warping.py:18-57),
 * monodepth loss map (utils/loss_functions.py:106-138), mean over the valid pixels — as row-walking strips: every input value is
 * loaded once, the 3x3 windows come from neighbouring lanes and from registers, no intermediate map touches HBM.  Bit for bit
 * what as_warp_fwd -> as_monodepth_loss_fwd -> as_masked_sum_mean and as_monodepth_loss_bwd_masked -> as_warp_bwd_add give.
 * pred [B,1,H,W]; left, right, warped [B,3,H,W]; mask uint8 [B,1,H,W]; out4 = {masked sum, count, mean, count}.
 * workspace: as_photometric_chain_workspace() floats, 16-byte aligned; the backward call takes the forward call's workspace as
 * fwd_workspace (per-image mean disparity) and its out4.  g_sum / g_mean: device scalars, either may be NULL. */
int64_t as_photometric_chain_workspace(int B, int H, int W);
int as_photometric_chain_fwd(const float* pred, const float* left, const float* right, int B, int H, int W,
                             float smoothness_weight, float* warped, uint8_t* mask, float* out4, float* workspace, void* stream);
int as_photometric_chain_bwd(const float* g_sum, const float* g_mean, const float* out4, const float* pred, const float* left,
                             const float* right, int B, int H, int W, float smoothness_weight, float* g_pred, float* workspace,
                             const float* fwd_workspace, void* stream);
/* The four loss maps from a given warped image, same strips (any output may be NULL); workspace as above. */
int as_monodepth_loss_rows_fwd(const float* pred, const float* img, const float* warped, int B, int H, int W,
                               float smoothness_weight, float* total, float* l1, float* ssim, float* smooth,
                               float* workspace, void* stream);

/* ---- loss[mask].mean() without a host sync — adapt.py:81-83 --------------------
 * out[0] = sum(v*m), out[1] = count(m); value = out[0]/out[1] is formed by the caller
 * on device.  workspace: as_masked_sum_workspace(n) floats. */
int64_t as_masked_sum_workspace(int64_t n);
int as_masked_sum(const float* v, const uint8_t* mask, int64_t n, float* out2, float* workspace, void* stream);
/* The same with out4 = [sum, count, sum / count, count]: the mean and a second copy of the count come out of the finalize
 * launch instead of two element-wise launches of the caller. */
int as_masked_sum_mean(const float* v, const uint8_t* mask, int64_t n, float* out4, float* workspace, void* stream);

/* ---- a13: khamis_robust_loss — utils/loss_functions.py:6-15 (ER modes, adapt.py:339-349) -------
 * out2[0] = sum_{gt>0}(sqrt((gt-pred)^2+4)/2 - 1) / max(count(gt>0),1), out2[1] = max(count,1).
 * as_khamis_bwd: g_pred = *g_loss * d out2[0] / d pred (g_loss: device scalar; out2 from the forward).
 * pred, gt: any shape with n elements.  workspace: as_khamis_workspace(n) floats, 8-byte aligned. */
int64_t as_khamis_workspace(int64_t n);
int as_khamis_fwd(const float* pred, const float* gt, int64_t n, float* out2, float* workspace, void* stream);
int as_khamis_bwd(const float* pred, const float* gt, const float* g_loss, const float* out2, int64_t n,
                  float* g_pred, void* stream);

/* ---- evaluation reductions — train.py:98-106 ------------------------------------
 * out6 = [sum |pred-gt| over gt>0, count(gt>0), count(gt>0 & |err|>2), >3, >4, >5]; EPE = out6[0]/out6[1],
 * D1_all_tpx = out6[t]/out6[1].  pred, gt: any shape with n elements.  workspace: as_eval_metrics_workspace(n). */
int64_t as_eval_metrics_workspace(int64_t n);
int as_eval_metrics(const float* pred, const float* gt, int64_t n, float* out6, float* workspace, void* stream);

/* ---- a12: clip_grad_norm_ + Adam, multi-tensor — adapt.py:208-210,391-393 ------
 * One flat fp32 arena holds params / grads / exp_avg / exp_avg_sq at equal offsets.
 * as_sumsq: out[0] = sum(g[0:n]^2) (deterministic two-stage).
 * as_adam_step: g is first multiplied by *grad_scale_dev (a device scalar, e.g. the clip
 * coefficient; NULL = 1), then the torch.optim.Adam update (no weight decay / amsgrad).  The step
 * count for the bias corrections is `step`, or *step_dev (a device float) when step_dev != NULL —
 * the latter lets a captured hipGraph replay successive steps. */
int64_t as_sumsq_workspace(int64_t n);
int as_sumsq(const float* g, int64_t n, float* out, float* workspace, void* stream);
/* coef[0] = min(max_norm / (sqrt(sumsq[0]) + 1e-6), 1): the scale clip_grad_norm_ applies (adapt.py:391). */
/* Glue of EdgeAwareRefinement's backward (stereo_net.py:116-121) as single launches:
 * as_relu_bwd: g_in[i] = out[i] > 0 ? g_out[i] : 0 (the final ReLU; n floats, 16-byte aligned);
 * as_mirror_taps_ch0: input channel 0 of a [32][Cin][3][3] weight with mirrored taps — by_tap [9][32] and by_channel [32][9]
 * (either may be NULL): the 32->1 data gradient of conv2d_feature towards the disparity channel. */
int as_relu_bwd(const float* g_out, const float* out, int64_t n, float* g_in, void* stream);
int as_mirror_taps_ch0(const float* w, int Cin, float* by_tap, float* by_channel, void* stream);
int as_clip_coef(const float* sumsq, float max_norm, float* coef, void* stream);
/* as_sumsq + as_clip_coef in the launches as_sumsq has anyway; step_counter (may be NULL) += 1: the optimizer's device-side
 * step count, read by as_adam_step under hipGraph replay. */
int as_sumsq_clip(const float* g, int64_t n, float max_norm, float* out, float* coef, float* step_counter,
                  float* workspace, void* stream);
int as_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                 const float* grad_scale_dev, float lr, float beta1, float beta2, float eps,
                 int step, const float* step_dev, void* stream);
/* as_adam_step with the learning rate read from *lr_dev (a device float): bit for bit as_adam_step at that lr; a captured step
 * follows a learning-rate schedule without a new capture. */
int as_adam_step_lr(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                    const float* grad_scale_dev, const float* lr_dev, float beta1, float beta2, float eps,
                    int step, const float* step_dev, void* stream);
/* The two above behind a device flag (`gate`, one int32): with *gate != 0 bit for bit as_sumsq_clip and as_adam_step (lr_dev
 * NULL) / as_adam_step_lr (lr_dev given); with *gate == 0 the parameters, both moments and the step counter stay untouched,
 * out and coef are still written.  An early return, never a wait. */
int as_sumsq_clip_gated(const float* g, int64_t n, float max_norm, float* out, float* coef, float* step_counter,
                        float* workspace, const int32_t* gate, void* stream);
int as_adam_step_gated(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                       const float* grad_scale_dev, float lr, const float* lr_dev, float beta1, float beta2, float eps,
                       int step, const float* step_dev, const int32_t* gate, void* stream);

/* ---- validated adaptation on the device — adapt.py:366-396, utils/stereo_reservoir.py ------------
 * as_adapt_gate: the three decisions of a step, by one wave.  Device inputs: fcs_smoothed, loss (fp32), batch_idx (int32),
 * u (fp64 in [0,1): the step's random number).  state = [size, offers, adds, updates] (int64), indices[capacity] (int32),
 * values[capacity] (fp32) persist; out3 = [novel, slot, update] (int32) is the step's output.
 *   novel = gate_enabled && (double)fcs_smoothed < threshold                  (strict: a NaN is never novel)
 *   novel: offers += 1; unless batch_idx is in indices[0:size]: size < capacity appends (slot = size, indices[size] =
 *          batch_idx, size += 1), else r = 1 + min((int64)(u * offers), offers - 1) and slot = r - 1 when r <= capacity (a
 *          replacement changes neither indices nor size, as the reference's reservoir); a slot: values[slot] = loss, adds += 1
 *   update = adapting && slot < 0; updates += update
 * as_reservoir_store: left and right (n floats each) into row *slot_dev of buf_left / buf_right ([capacity][n]); no write
 * at all when the slot is < 0 or >= capacity.  16-byte accesses where both sides are 16-byte aligned. */
int as_adapt_gate(const float* fcs_smoothed, const float* loss, const int32_t* batch_idx, const double* u,
                  double threshold, int capacity, int gate_enabled, int adapting, int64_t* state,
                  int32_t* indices, float* values, int32_t* out3, void* stream);
int as_reservoir_store(const float* left, const float* right, int64_t n, const int32_t* slot_dev, int capacity,
                       float* buf_left, float* buf_right, void* stream);

/* ---- the K best pairs of a stream on the device — utils/stereo_priority_queue.py ---------------------
 * as_pq_offer: one offer to a queue that keeps the `capacity` smallest keys, by one wave.  Device inputs: value (fp32), index
 * (int32).  key = value for min_heap != 0, else -value (fp32, exact).  state = [size, offers, adds] (int64, 8-byte aligned),
 * indices[capacity] (int32) and keys[capacity] (fp32) persist; rows [0, size) are the members, in no particular order.
 *   offers += 1
 *   refused (out_slot = -1, nothing else written) when index is in indices[0:size]
 *   size < capacity: out_slot = size, size += 1
 *   else: the worst member is the maximum by (key, index); out_slot = its row when key < its key (strictly), else -1
 *   a slot: indices[slot] = index, keys[slot] = key, adds += 1
 * One deviation from the reference, ours: a NaN value is always refused (the reference's heap would keep it below capacity and
 * lose its order).  as_reservoir_store with out_slot as its slot_dev then copies the pair into the row. */
int as_pq_offer(const float* value, const int32_t* index, int capacity, int min_heap, int64_t* state, int32_t* indices,
                float* keys, int32_t* out_slot, void* stream);

/* ---- supervised two-scale loss — train.py:215, utils/loss_functions.py:18-38 with scales = [s, s + k] ----------
 * pred0 = pred_disp_l/s, up = pred_disp_l/(s+k) (the up-sampled coarse map), gt: n elements each.  One pass over gt:
 * out4 = [khamis(pred0, gt), khamis(up, gt), out4[0] + out4[1] (fp32), max(count(gt > 0), 1)]; NaN in gt is not valid.
 * workspace: as_khamis2_workspace(n) floats, 8-byte aligned.  Deterministic (fixed-order fp64 sums).
 * as_khamis2_bwd: g_out3 = device gradients of out4[0..2].  g_pred0 [B,1,H,W] = (g_out3[0] + g_out3[2]) / out4[3] * d value /
 * d pred0; g_coarse [B,h,w] = gain * (bilinear up-sampling adjoint, align_corners=False) of (g_out3[1] + g_out3[2]) / out4[3] *
 * d value / d up, the derivative map formed where the adjoint loads it.  gain is the forward's (2^k), not W / w.  Ratios W / w
 * beyond the adjoint's span are refused as by as_upsample_bilinear_bwd. */
int64_t as_khamis2_workspace(int64_t n);
int as_khamis2_fwd(const float* pred0, const float* up, const float* gt, int64_t n, float* out4, float* workspace,
                   void* stream);
int as_khamis2_bwd(const float* pred0, const float* up, const float* gt, const float* g_out3, const float* out4,
                   int B, int H, int W, int h, int w, float gain, float* g_pred0, float* g_coarse, void* stream);

/* ---- the proxy-label term of the adaptation loss — sgm.ProxyLabeler's outputs, read where they lie -------------
 * pred: the network's disparity; disp: the matcher's left map (as_sgm_select's disp_l); code: the final code of the chain
 * (as_disp_speckle's code).  fp32 / fp32 / uint8, n elements each, any shape; code may start at any byte.
 * A pixel carries a label iff code[i] == 0 && disp[i] > 0.f: NaN, -0.0, 0.0, negatives and every non-zero code carry none.  This is
 * the set where(code == 0, disp, 0) > 0, the valid set of as_khamis_fwd on the materialised labels.
 * as_proxy_term_fwd: one streaming launch and a one-wave finalize; every output overwritten on every call, nothing read back.
 *   v[i] = sqrt((disp - pred)^2 + 4) / 2 - 1 in fp32, the chain of as_khamis_fwd bit for bit (csrc/khamis.h: fma(d, d, 4), the
 *     hardware's square root, fma(s, 0.5, -1));  e[i] = |disp[i] - pred[i]| (fp32, exact)
 *   S = sum v, C = count, E = sum e, B = count(e > bad_px) over the labelled pixels: fp64, fixed order, two stages, with the
 *     partition and the order of as_khamis_fwd (min(ceil(n / 256), 512) workgroups of 256, element i in lane i % 256 of
 *     workgroup (i / 256) % workgroups, rising i per lane, the wave sum, the four waves, then one wave over the workgroups)
 *   out6 = [ (float)S / (float)max(C, 1),  (float)max(C, 1),  (float)S,  (float)(E / max(C, 1)),  (float)(B / max(C, 1)),  (float)C ]
 *   out6[0], out6[1] are bit for bit as_khamis_fwd's out2 on where(code == 0, disp, 0); without a label out6 = [0, 1, 0, 0, 0, 0].
 *   A NaN of pred shows only where the pixel is labelled.  bad_px: finite, >= 0.
 *   workspace: as_proxy_term_workspace(n) floats, 8-byte aligned (-1 for n <= 0).
 * as_proxy_term_bwd: one launch.  g_pred[i] = *g_loss / out6[1] * d v[i] / d pred[i] = -scale * d / (2 sqrt(d^2 + 4)) with
 *   d = disp - pred on the labelled pixels (the expression of as_khamis_bwd, compiled like it without contraction: every
 *   operation rounded once, IEEE division and square root; bit for bit its result on the materialised labels),
 *   exactly 0.f elsewhere.  g_loss: device scalar; out6: the forward's.  16 bytes per lane where pred, disp and g_pred are 16-byte
 *   aligned, element by element otherwise and for the last n % 4.
 * Refused (error set, nothing launched): a null pointer, n <= 0, an fp32 argument off 4 bytes, a workspace off 8 bytes, bad_px
 * negative or not finite, out6 or workspace sharing a byte with an input or each other, g_pred sharing a byte with an input. */
int64_t as_proxy_term_workspace(int64_t n);
int as_proxy_term_fwd(const float* pred, const float* disp, const uint8_t* code, int64_t n, float bad_px, float* out6,
                      float* workspace, void* stream);
int as_proxy_term_bwd(const float* pred, const float* disp, const uint8_t* code, const float* g_loss, const float* out6,
                      int64_t n, float* g_pred, void* stream);

/* ---- dataset layer on the device ----------------------------------------------------
 * What datasets/stereo_dataset.py:49-96 and utils/dataset_utils.py:26-57 do per sample on the host (ToTensor,
 * flip_stereo_pair, crop, disparity decoding), over the raw decoded file contents uploaded once:
 * as_decode_rgb8: src = uint8 [H0][W0][3] (PIL RGB) -> dst = float [3][H][W] = src/255 of the window (i0, j0, H, W);
 *   hflip = 1: the image was mirrored BEFORE cropping (the caller also swaps left and right, dataset_utils.py:19-23).
 * as_decode_plane: one-channel sample -> float [H][W]; dtype 0 = f32, 1 = u16, 2 = u8; vflip = 1 for bottom-up
 *   files (PFM, utils/io.py:73); value = v*scale (KITTI png 1/256, KITTI-raw npy 1/128, PFM 1) or scale/v
 *   (reciprocal = 1: Virtual KITTI depth in cm -> disparity, scale = baseline*focal/0.01).
 * The multi-scale pyramid (stereo_dataset.py:98-135) is as_upsample_bilinear_fwd (a general align_corners=False
 * resize) with gain 1 for colour and 1/2^s for disparity. */
int as_decode_rgb8(const uint8_t* src, int H0, int W0, int i0, int j0, int H, int W, int hflip, float* dst,
                   void* stream);
int as_decode_plane(const void* src, int dtype, int H0, int W0, int i0, int j0, int H, int W, int hflip,
                    int vflip, float scale, int reciprocal, float* dst, void* stream);

/* ---- depth and point cloud from disparity (csrc/pointcloud.hip) — ros/stereo_depth_node.py:145-195 ----------
 * What the reference's ROS node computes on the host (F.interpolate to pyramid level s, depth = fx*b/disp, clamp,
 * Open3D's 16-bit depth image, pinhole back-projection, voxel_down_sample, the x,y,z,rgb records of
 * ros/open3d_to_ros.py:15-22,57).  disp [B,1,H,W] is full-resolution disparity in pixels, rgb [B,3,H,W] in [0,1]
 * (may be NULL); n = 2^s, h = H >> s, w = W >> s (trailing rows and columns of a ragged size are unused).
 * Every fp32 expression is a sequence of single IEEE operations in the written order (no fma):
 *   m      = ((a + b) + (c + d)) * 0.25f over source pixels (n*v+o, n*u+o), (.., +1), (+1, ..), (+1, +1), o = n/2 - 1;
 *            m = disp[v,u] for s = 0.  Colour: the same pixels and formula per channel.
 *   depth  = fminf(fb / m, max_depth), negative -> 0, NaN stays NaN (the pixel is invalid)
 *   q      = (int)(depth * depth_scale), z = (float)q / depth_scale; invalid when q == 0 or z > depth_trunc.
 *            depth_scale == 0: z = depth, invalid unless 0 < z <= depth_trunc.
 *   x      = (((float)u - cxs) * z) / fxs,  y = (((float)v - cys) * z) / fys
 *   voxel  ix = (int)floorf(x / voxel_size) (iy, iz likewise), anchored at the camera origin; a point with an |i| >= 2^20
 *            is counted in dropped[b] and not inserted.  Per voxel, all integers: count, Sx/Sy/Sz += llrintf(coord *
 *            65536.f) (64 bit), Sr/Sg/Sb += (int)(colour * 255.f) clamped to 0..255.
 *   record X = (float)((double)Sx / ((double)count * 65536.0)) (Y, Z likewise), R = Sr / count: 16 bytes x, y, z fp32 and
 *            a u32 R << 16 | G << 8 | B (0 without colour).  Integer sums: a voxel's record does not depend on arrival order.
 * The camera holds fp32 values rounded once on the host from full-resolution intrinsics: fb = fx * baseline, fxs = fx / n,
 * fys, cxs, cys likewise.  max_depth * depth_scale <= 65535.
 *
 * as_voxel_table_slots: default slot count for that many points per image: a power of two >= 2 * points, >= 1024.
 * as_voxel_table_bytes: size of the table workspace (16-byte aligned) for B images of `slots` slots.
 * as_voxel_table_clear: empties a table.  ONCE after allocation: as_voxel_cloud_finalize hands every slot it read back
 *   empty, so call-to-call independence costs no pass over the table; a frame never sees an earlier frame's voxels as long
 *   as every as_disp_to_points with a table is followed by its finalize (clear again after abandoning a frame in between).
 * as_disp_to_points: one pass over the frame.  depth_out [B,1,h,w] (the clamped depth, before quantisation), xyz_out
 *   [B,3,h,w] (x, y, z planes, NaN at invalid pixels) and table may each be NULL.  With a table every valid point is
 *   inserted into its image's open-addressing hash table (64-bit key of three biased 21-bit indices, atomicCAS on the key,
 *   linear probing bounded by `slots` probes — a point that finds no slot is counted in dropped[b] — then integer
 *   atomicAdds).  slots: a power of two >= max(64, h*w); voxel_size in (0, 16]; B <= 65535.
 * as_voxel_cloud_finalize: compacts the occupied slots of image b into rows [0, n[b]) of records [B][cap] (16 bytes each,
 *   16-byte aligned), voxel [B][cap][3], count [B][cap]; n [B] and dropped [B] are overwritten.  Rows at or beyond n[b]
 *   are left untouched, the order of rows within an image is unspecified; voxels beyond cap are counted in n[b] but not
 *   written (cap = h*w always suffices). */
typedef struct as_depth_camera {
  float fb;                       /* float32(fx * baseline) */
  float fxs, fys, cxs, cys;       /* float32(fx / n) ... at pyramid level s */
  float max_depth, depth_scale, depth_trunc;
} as_depth_camera;
int64_t as_voxel_table_slots(int64_t points_per_image);
int64_t as_voxel_table_bytes(int B, int64_t slots);
int as_voxel_table_clear(void* table, int B, int64_t slots, void* stream);
int as_disp_to_points(const float* disp, const float* rgb, int B, int H, int W, int s, const as_depth_camera* cam,
                      float* depth_out, float* xyz_out, float voxel_size, void* table, int64_t slots, void* stream);
int as_voxel_cloud_finalize(void* table, int B, int64_t slots, int cap, void* records, int32_t* voxel, int32_t* count,
                            int32_t* n, int32_t* dropped, void* stream);
/* as_disp_to_points_gated: as_disp_to_points with a confidence gate; everything not named here is as_disp_to_points', from the
 * same device code.  conf [B][h][w] (required, dense fp32, at the pyramid level's OWN resolution h = H >> s, w = W >> s);
 * conf_min must not be NaN (-inf keeps every pixel with a number for a confidence).
 *   gate      a pixel that is valid by the depth rules above is kept only when conf[b][v][u] >= conf_min (one fp32 compare; a
 *             NaN confidence fails it, +inf passes).  A rejected pixel is NaN (0x7FC00000) in all three planes of xyz_out and
 *             is not inserted into the table; the index-range check runs after the gate, so it is not counted in dropped[b]
 *             either.  depth_out is written as before for EVERY pixel.
 *   rejected  NULL or [B] int32, OVERWRITTEN: the number of pixels of image b that were valid by depth and failed the gate
 *             (zeroed on the stream in front of the launch, then one counter add per wave from a ballot; integers: exact).
 * Everything is enqueued on the caller's stream: allocates nothing, never waits, capturable. */
int as_disp_to_points_gated(const float* disp, const float* rgb, const float* conf, float conf_min, int B, int H, int W, int s,
                            const as_depth_camera* cam, float* depth_out, float* xyz_out, float voxel_size, void* table,
                            int64_t slots, int32_t* rejected, void* stream);

/* ---- per-pixel disparity confidence and binned error statistics (csrc/confidence.hip) — no counterpart in the reference ------
 * as_disp_confidence: one launch over logits [B][D][H][W] (dense fp32, as as_softargmax_fwd reads it), 1 <= D <= 64, B <= 65535,
 * H * W <= 2^30.  Outputs [B][H][W], each may be NULL (at least one is not).  A bad argument returns AS_ERR_ARG before any launch.
 * No atomics, no workspace; allocates nothing, never waits, capturable.  Compiled with `#pragma clang fp contract(off)`: every
 * expression below is a sequence of single IEEE fp32 operations in the written order.  Per pixel, x_d its D logits:
 *   maximum   m1 and a = the maximum and the FIRST index attaining it: `if (x_d > m1) { m1 = x_d; a = d; }` over d in increasing
 *             order from m1 = -inf, a = 0.  For finite columns the index as_softargmax_fwd's argmax gives.
 *   exps      t_d = x_d - m1, e_d = expf(t_d), se = the sum of e_d in increasing d from 0.f: as_softargmax_fwd's se.
 *   pmax      1.f / se: the soft-max probability of the mode.
 *   mass      ((e_{a-1} + e_a) + e_{a+1}) / se, a neighbour outside [0, D) contributing 0.f: the probability within one coarse
 *             disparity of the mode.
 *   cent      1.f - Hn / logf((float)D), then fminf(fmaxf(., 0.f), 1.f); Hn = logf(se) - T / se; T = the sum in increasing d
 *             from 0.f of (e_d == 0.f ? 0.f : e_d * t_d), each product rounded on its own.  One minus the normalised entropy.
 *   D == 1    all three maps are 1.f.
 *   bad       a column holding a NaN or a +inf, or consisting only of -inf, is the quiet NaN 0x7FC00000 in every map (for every
 *             D, 1 included).  A -inf among finite values is legal: probability 0.
 *
 * as_sparsification: error statistics of pred against gt, binned by a key map.  key, pred, gt: n fp32 elements each, any shape;
 * 1 <= n <= 2^40, 1 <= K <= 1024, lo finite, scale positive and finite (the caller's float(K / (hi - lo)), rounded once on the
 * host), tau not NaN; count [K], bad [K], skipped [1] int64 and abs_err [K] fp64, 8-byte aligned.  Per element, in fp32:
 *   !(gt > 0)            ignored, as in as_eval_metrics.
 *   err = fabsf(pred - gt).  key or err NaN: *skipped += 1 and nothing else.
 *   t = (key - lo) * scale (two single operations); k = t < 0 ? 0 : (t >= (float)K ? K - 1 : (int)t).
 *   count[k] += 1;  bad[k] += err > tau;  abs_err[k] += (double)err.
 * All four outputs ACCUMULATE (the caller zeroes them): batches add up, and a captured call appends on every replay.  The
 * integers are exact.  abs_err is an fp64 sum in an unspecified order (per-workgroup partial sums, then atomics): it differs
 * from the exact sum by at most n 2^-53 times the bin's sum.  Allocates nothing, never waits, capturable. */
int as_disp_confidence(const float* logits, int B, int D, int H, int W, float* pmax, float* cent, float* mass, void* stream);
int as_sparsification(const float* key, const float* pred, const float* gt, int64_t n, float lo, float scale, int K, float tau,
                      int64_t* count, int64_t* bad, double* abs_err, int64_t* skipped, void* stream);

/* ---- per-image feature-contrast scores (csrc/ood.hip) — evaluation/ood_analysis.py:76-77, utils/feature_contrast.py ------
 * One pass over logits [B][D][H][W] (dense fp32, as as_softargmax_fwd reads it), 1 <= D <= 64 (more: AS_ERR_ARG before any
 * launch), B <= 65535.  Outputs, each may be NULL (at least one is not):
 *   fcs_mean [B][H][W]    m1 - (sum - m1 - m2) / (float)(D - 2) for D > 2, else 0: sum = fp32 sum of the D values in increasing
 *                         d starting from 0.f; m1, m2 = the largest and second largest (`if (v > m1) { m2 = m1; m1 = v; } else
 *                         if (v > m2) m2 = v;` from -inf, -inf).  Expression for expression the fcs of as_softargmax_fwd: the
 *                         same bits for finite logits.
 *   fcs_median [B][H][W]  m1 - e, e = the element of rank (D - 1) / 2 (integer division) when the D values are put in ascending
 *                         order, equal values in order of d: torch.median's lower median.  One fp32 subtraction of two inputs.
 *   A pixel with a NaN among its D values is NaN (0x7FC00000) in both maps, for every D.
 *   scores                row r = (cursor ? *cursor : 0) + b holds, when 0 <= r < capacity, two floats at scores + 2 * r:
 *                         (float)(S / (double)(H * W)) with S the fp64 sum of the image's mean map, then the same of its median
 *                         map.  S is summed in a fixed order (lane t of 512: pixels t, t + 512, ... in order; xor butterfly over
 *                         the 64 lanes of a wave, offsets 32 down to 1; the 8 waves in order): no atomics, no workspace, the same
 *                         bits on every run.  Rows outside [0, capacity) are not written.
 *   cursor, dropped       device int32, each may be NULL, both NULL without scores.  After the rows are written, in stream order
 *                         (a second, one-lane launch): *dropped += the number of rows of this call that were not written;
 *                         *cursor += B (saturating at INT32_MAX - 65535; a negative cursor is left alone).  A captured graph
 *                         that contains the call appends on every replay. */
int as_fcs_scores(const float* logits, int B, int D, int H, int W, float* fcs_mean, float* fcs_median, float* scores,
                  int capacity, int32_t* cursor, int32_t* dropped, void* stream);

/* ---- per-image entropy of intensities and horizontal differences (csrc/entropy.hip) — utils/entropy.py:11-21,31-44 ------
 * One pass over img [B][C][H][W] (dense fp32).  Per image b, over its whole [C][H][W] block (the reference flattens whatever it
 * is given), all in integers:
 *   v            (int32)(255.0f * x): the product rounded to fp32, then truncated toward zero (x = -0.001 gives v = 0).
 *                The reference's .int() is undefined for what follows, so this rule is OURS: a pixel whose product is NaN,
 *                +-inf or of magnitude >= 2^31 is INVALID; it enters no bin and no difference it takes part in enters one.
 *   count_g[v]   += 1 for 0 <= v <= 255; other values are ignored (torch.histc(min=0, max=255) ignores them).
 *   count_d[q]   += 1 for d = v[y][x+1] - v[y][x] inside a row of a plane (never across a row end, a plane or an image; v not
 *                range-limited) with -255 <= d <= 255 and q = min((d + 255) * 256 / 510, 255) in integer division; other
 *                differences are ignored.
 *   scores       row r = (cursor ? *cursor : 0) + b holds, when 0 <= r < capacity, two floats at scores + 2 * r:
 *                (float)(-S) with S = the fp64 sum over bins 0..255 in that order, from 0.0, of p * log2(p) for every count > 0,
 *                p = (double)count / (double)N; column 0: count_g and N = H * W, column 1: count_d and N = H * (W - 1).  N is the
 *                PLANE's size for every C, as the reference divides by shape[-2] * shape[-1].  W == 1: column 1 is NaN
 *                (0x7FC00000), the reference's 0 / 0.  Integer counts and a fixed order: the same bits on every run.
 *   hist         NULL or [B][2][256] uint32: count_g then count_d of image b (indexed by b, not by the cursor).
 *   cursor, dropped   exactly as_fcs_scores' (a second, one-lane launch); each may be NULL.
 * workspace: as_image_entropy_workspace(B) bytes (0 for a B outside [1, 65535]), 4-byte aligned, ALL ZERO before its first
 * use; every call leaves it all zero again (the last workgroup of an image zeroes that image's slice), so a captured graph
 * needs no memset node.  A workspace serves one call at a time.  B <= 65535, C * H * W <= 2^30, capacity >= 1; a bad argument
 * returns AS_ERR_ARG before any launch.  Allocates nothing, never waits, capturable. */
int64_t as_image_entropy_workspace(int B);
int as_image_entropy(const float* img, int B, int C, int H, int W, float* scores, int capacity, int32_t* cursor,
                     int32_t* dropped, uint32_t* hist, void* workspace, void* stream);

/* ---- cost-volume probe: extreme-contrast pixels and rank profile (csrc/cv_probe.hip) — evaluation/cost_volume_analysis.py:82-92 ----
 * One pass over logits [B][D][H][W] (dense fp32, the tensor as_fcs_scores reads), 1 <= D <= 64, B <= 65535, H * W <= 2^30,
 * capacity >= 1; gt NULL or [B][1][H][W] fp32 (the coarse ground truth).  A bad argument returns AS_ERR_ARG before any launch.
 * Allocates nothing, never waits, capturable.  Compiled with `#pragma clang fp contract(off)`: every expression below is a
 * sequence of single IEEE fp32 operations in the written order.
 *   map f        per pixel p = row * W + col, as_fcs_scores' fcs_mean: `sum += v; if (v > m1) { m2 = m1; m1 = v; } else if
 *                (v > m2) m2 = v;` over d in increasing order from sum = 0.f, m1 = m2 = -inf; mean_rest = (sum - m1 - m2) /
 *                (float)(D - 2) and f = m1 - mean_rest for D > 2; f = 0 for D <= 2; f = NaN when any of the D values is NaN.  For
 *                finite logits the same bits as as_fcs_scores and as_softargmax_fwd give.
 *   selection    torch's argmax (which = 0, "hi") and argmin (which = 1, "lo") of the flattened map: the smallest p whose f is NaN
 *                if any pixel's is (both times), otherwise the smallest p with f[p] == the extreme.  Values compare as fp32 numbers
 *                (-0.f equals +0.f).  The reduction carries (value, p) and breaks value ties on p, never on a lane number.
 * Row r = (cursor ? *cursor : 0) + b is written when 0 <= r < capacity.  Outputs, each may be NULL (at least one is not; a NULL
 * output is not written):
 *   pix     [capacity][2][3] int32   row, col, d_max (the smallest d holding m1; -1 at a NaN pixel)
 *   vals    [capacity][2][5] fp32    f, m1, m2, mean_rest, gt[b][row][col].  The gt entry is NaN without gt; D <= 2: mean_rest is
 *                                    NaN (and m2 is -inf for D == 1); at a NaN pixel m1, m2 and mean_rest are NaN; every such NaN
 *                                    is 0x7FC00000.  In every other case f == m1 - mean_rest bit for bit.
 *   slices  [capacity][2][D] fp32    the D logits of the pixel, copied bit for bit
 *   profile [capacity][D] fp32       profile[r][j] = (float)(S_j / (double)(H * W)), S_j the fp64 sum over the image's pixels of the
 *                                    j-th largest of the pixel's D values (j = 0 is the maximum).  A pixel holding a NaN makes every
 *                                    S_j of its image NaN.  No floating-point atomics; the order of the sum is a function of the
 *                                    shape only, so the same input gives the same bits on every run (the order itself is not part
 *                                    of the contract).
 *   cursor, dropped                  exactly as_fcs_scores' (a second, one-lane launch); each may be NULL. */
int as_cost_volume_probe(const float* logits, const float* gt, int B, int D, int H, int W, int32_t* pix, float* vals,
                         float* slices, float* profile, int capacity, int32_t* cursor, int32_t* dropped, void* stream);

/* ---- LiDAR ground truth: Velodyne scan -> sparse depth and disparity (csrc/lidar.hip) — scripts/export_gt_disp.py:86-115,156-162 ----
 * What the reference's export script computes on the host per frame: the scan is projected into a rectified camera, the nearest
 * return is kept per pixel, depth becomes disparity = baseline * fx / depth and is stored as uint16 = 128 * disp.
 * points [B][Nmax][4] fp32 in KITTI .bin layout (x forward, y left, z up, reflectance; 16-byte aligned), counts [B] int32 ON THE
 * DEVICE (a captured graph replays scans of different lengths; lanes at or beyond min(counts[b], Nmax) read nothing, 0 is legal),
 * P [B][3][4] fp64 row-major (velodyne -> image: P_rect_0c . R_rect_00 (4x4) . [R|T], composed on the host), zbuf [B][H][W] uint32.
 *
 * as_lidar_project, per point, in fp64, every expression a sequence of single IEEE operations in the written order (no fma):
 *   keep     x >= 0 (fp32 compare: keeps -0.0, drops NaN); the point is (x, y, z, 1), its fourth word is never used
 *   q_k    = ((P[k][0] * x + P[k][1] * y) + P[k][2] * z) + P[k][3]            k = 0, 1, 2
 *   u      = rint(q0 / q2) - 1.0, v = rint(q1 / q2) - 1.0     round half to even, as np.round; there is NO test of q2 > 0: a
 *            point behind the camera that lands in bounds is kept, as in the reference
 *   keep     0 <= u < W and 0 <= v < H, compared in fp64 (inf and NaN fail them as they do in numpy)
 *   value  = x (the fp32 input) when vel_depth, else (float)q2 (round to nearest)
 *   key    = the value's bits with the sign bit flipped when the value is positive, all bits flipped when it is negative: unsigned
 *            order = float order (-0.0 just below +0.0), so a negative q2 wins the minimum and the pixel resolves to depth 0
 *   zbuf[b][v][u] = min(zbuf[b][v][u], key) by atomicMin.  The empty key is 0xFFFFFFFF (no value encodes to it).  An integer
 *            minimum does not depend on arrival order: the buffer is deterministic.
 * The reference finds duplicates through a linear index row * (W - 1) + col - 1, which pixel (r, W-1) shares with pixel (r+1, 0);
 * this keeps the minimum PER PIXEL, what the comment there says.  Only columns 0 and W-1 can differ from the reference.
 *
 * as_lidar_resolve, one pass over zbuf, per pixel of the window (i0, j0, h, w) inside H x W:
 *   depth  = 0 for an empty key, else the decoded value, and 0 where that is < 0 (-0.0 stays -0.0, as in the reference)
 *   disp64 = bf / (double)depth in fp64, bf = baseline * fx as fp64; 0 where depth == 0 or depth > 80 (fp32 compares).  The
 *            reference divides an np.float64 scalar by a float32 array, which numpy >= 2 (checked with 2.2.6) promotes to float64,
 *            so its division and its * 128.0 are fp64 as well.
 *   q      = (uint16)trunc(128.0 * disp64).  Where 128.0 * disp64 > 65535 the reference asserts; here the pixel is 0 in EVERY
 *            output (depth too) and is counted in overflow[b].
 *   disp   = (float)q / 128.f when quantize (bit for bit what as_decode_plane yields from the exported file), else (float)disp64.
 * Outputs, each may be NULL: depth_out [B][1][h][w] fp32, disp_out [B][1][h][w] fp32, disp_u16 [B][h][w], overflow [B] int32
 * (overwritten; integer atomics).  pred [B][1][h][w] fp32 (may be NULL) comes with metrics [B][6] and workspace
 * (as_lidar_resolve_workspace(B, H, W) BYTES, 8-byte aligned): row b of metrics has the layout of as_eval_metrics' out6 over the
 * window's pixels with disp > 0 of image b, |pred - disp| and the strict > 2, 3, 4, 5 in fp32.  No float atomics: each
 * workgroup of 256 consecutive pixels writes six fp64 partials (xor butterfly over the wave, offsets 32 down to 1, then the four
 * waves in order); one wave per image adds them (lane t: blocks t, t + 64, ... in order, then the butterfly) and rounds to fp32
 * once.  Counts are exact, a replay gives the same bits.
 * The pass reads EVERY pixel of zbuf, outside the window too, and hands each key it read back empty: call-to-call independence
 * costs no pass of its own.  as_lidar_zbuf_clear empties the buffer ONCE after allocation; clear again after abandoning a frame
 * between its project and its resolve (the contract of the voxel table above).  B <= 65535, H * W < 2^30. */
int as_lidar_zbuf_clear(uint32_t* zbuf, int B, int H, int W, void* stream);
int as_lidar_project(const float* points, const int32_t* counts, const double* P, int B, int Nmax, int H, int W, int vel_depth,
                     uint32_t* zbuf, void* stream);
int64_t as_lidar_resolve_workspace(int B, int H, int W);
int as_lidar_resolve(uint32_t* zbuf, int B, int H, int W, int i0, int j0, int h, int w, double bf, int quantize,
                     float* depth_out, float* disp_out, uint16_t* disp_u16, const float* pred, float* metrics, void* workspace,
                     int32_t* overflow, void* stream);

/* ---- colour-mapped disparity and error images (csrc/visualize.hip) — utils/visualization.py ------------------------------
 * What the reference computes on the host per image (apply_cmap :115-158 through matplotlib's Colormap.__call__, then
 * float_image_to_cv_uint8 :161-178): x [B][1][H][W] fp32, or |y - x| formed on the fly when y is not NULL, is normalised per image
 * and looked up in a table.  B <= 65535, B*H*W <= 2^30.
 *
 * The arithmetic, every operation a single IEEE fp32 operation in the written order:
 *   v   = x, or fabsf(y - x)
 *   lo, den: `automatic` is a mask, bit 0 = lo is the minimum of the image's v, bit 1 = hi is its maximum (both as torch.min /
 *         torch.max: a NaN in the image is a NaN in both).  automatic == 0: lo and den are used as passed and hi is ignored —
 *         the caller passes lo = (float)vmin, den = (float)((double)vmax - (double)vmin), which is what the reference's Python
 *         floats give and NOT (float)vmax - (float)vmin.  Otherwise the fixed one of lo, hi is used as passed, den = hi - lo and
 *         the passed den is ignored.
 *   n   = (v - lo) / den        a correctly rounded division, never a multiplication by a reciprocal
 *   t   = n * (float)N
 *   idx = N + 2 (bad) when t is NaN; N - 1 when t == N; N (under) when t < 0; N + 1 (over) when t > N; else (int)t.
 *   So -0.0 is entry 0, a constant image with automatic bounds is 0/0 = bad in every pixel (the reference's black image), an
 *   image holding +inf with automatic bounds has its finite pixels at entry 0 and the infinite one bad.
 * table: device pointer to N + 3 entries (1 <= N <= 256; then under, over, bad), 4-byte aligned, copied to LDS by every
 *   workgroup: uint8 [N+3][4] (r, g, b, unused) for the u8 modes, fp32 [N+3][4] (r, g, b, a) for f32; may be NULL for index.
 * mode and out:
 *   0  u8 RGB   out [B][H][W][3] uint8, 4-byte aligned (AS_ERR_ARG otherwise).  The batch is ONE byte stream stored in whole
 *   1  u8 BGR   dwords; image b starts at byte b*H*W*3, which is odd for odd H*W, and a dword that straddles two images carries
 *               each image's own range.
 *   2  f32      out [B][3][H][W] fp32 planes r, g, b
 *   3  index    out [B][H][W] int16 = idx
 * as_colormap_range writes P = min(64, ceil(H*W / 4096)) (min, max) fp32 pairs per image into workspace
 * (as_colormap_workspace(B, H*W) BYTES, 4-byte aligned; -1 for a shape outside the limits): no float atomics, and no finalize
 * launch — as_colormap_apply folds the P pairs of an image itself.  A call with both bounds fixed is one launch, one with an
 * automatic bound is as_colormap_range + as_colormap_apply with the same x, y and shape; neither synchronises.
 *
 * as_image_to_cv: the conversions without a colour map (tensor_to_cv_rgb :47-58, _gray :61-72, _disp :25-44).
 *   in [B][C][H][W] fp32, C = 1 or 3 -> out [B][H][W][C], channels reversed when flip (RGB -> BGR).
 *   t = 255.0f * v; when div != 0, t = t / div (a second, separately rounded operation; tensor_to_cv_disp passes (float)W).
 *   out_f32: out holds t as fp32.  Otherwise uint8 = trunc(t) SATURATED to 0 .. 255, NaN = 0: the reference's
 *   astype(np.uint8) is unspecified outside 0 .. 255 (it wraps on some hosts), so only in-range values are comparable.
 *   out 4-byte aligned; B*H*W*C <= 2^30. */
int64_t as_colormap_workspace(int B, int64_t pixels_per_image);
int as_colormap_range(const float* x, const float* y, int B, int H, int W, void* workspace, void* stream);
int as_colormap_apply(const float* x, const float* y, int B, int H, int W, int automatic, float lo, float hi, float den,
                      const void* workspace, const void* table, int N, int mode, void* out, void* stream);
int as_image_to_cv(const float* in, int B, int C, int H, int W, int flip, float div, int out_f32, void* out, void* stream);

/* ---- both-view inference: mirrored batches, left-right consistency check, background fill (csrc/lr_consistency.hip) ----
 * The reference's predict_disparity_leftright (adapt.py:40-62) runs the network once over [left; flip(right)] and
 * [right; flip(left)]: the second half of the output is the right view's disparity, mirrored in x.  The check keeps a pixel only
 * if the pixel it maps to in the other view maps back; the fill replaces the rest from the background.  tests/lr_consistency_ref.py
 * restates the three contracts below in numpy float32.  All maps are dense fp32 [B][1][H][W] unless stated; every entry point is
 * stream-ordered, allocates nothing and reads nothing back (capturable).  AS_ERR_ARG, before anything is enqueued, for a NULL
 * required pointer, a non-positive extent or an extent beyond what the kernel indexes (named in as_last_error).
 *
 * as_mirror_pair: one launch.  left, right [B][C][H][W] -> left_batch [2B][C][H][W] = [left ; right mirrored in x],
 *   right_batch [2B][C][H][W] = [right ; left mirrored in x], "mirrored" being m[b][c][y][x] = v[b][c][y][W-1-x].  Data movement
 *   only.  Four elements per lane when W % 4 == 0 and all four bases are 16-byte aligned, two when W % 2 == 0 and they are
 *   8-byte aligned, one otherwise; the outputs may alias neither each other nor an input.
 * as_flip_w: dst[p][y][x] = src[p][y][W-1-x] over `planes` planes of H x W, out of place (dst != src); the same three routes.
 *
 * as_lr_check: one kernel launch (and a small clearing launch when counts is given: a kernel, because a memset node was seen to
 *   fill with a stale pattern from the second replay of a captured graph on) for both views.  Every output pointer is optional
 *   (NULL: not written, not touched), at least one must be given.  mirrored = 1: disp_r is the map as the network produced it for
 *   the mirrored pair, i.e. element [b][y][W-1-x] holds the right view's pixel x; the kernel indexes it that way and every output
 *   is in the ordinary (unmirrored) layout, bit-identical to mirrored = 0 on the flipped-back map.  Below, R[x] and L[x] are the
 *   right and left view's row y of image b in the ordinary layout.  tol_abs, tol_rel: finite, >= 0.  W <= 2^24, B <= 65535.
 *   The left view at (b, y, x), in fp32, every operation rounded once and none contracted:
 *     1  d = L[x].  !(d >= 0) or d == +inf: code 4 (bad input).
 *     2  u = (float)x - d.  u < 0: code 3 (out of view).
 *     3  i0 = (int)floorf(u), i1 = min(i0 + 1, W - 1), t = u - (float)i0, a = R[i0], b = R[i1].
 *     4  r = (t == 0) ? a : a + t * (b - a): the subtraction, the product and the sum each rounded once.  With t == 0 the
 *        neighbour b does not enter, so a NaN there does not reach r.
 *     5  r not finite, or r < 0: code 4.
 *     6  e = fabsf(d - r), tol = fmaxf(tol_abs, tol_rel * d).
 *     7  code 0 (consistent) if e <= tol; else 1 (occluded) if r > d: something nearer covers the pixel; else 2 (mismatch).
 *   The right view at (b, y, x) is the mirror statement: d = R[x]; u = (float)x + d; out of view if u > (float)(W - 1); a and b
 *   are taken from L.
 *   code_l, code_r: uint8.  valid_l, valid_r: fp32, 1.0 where the code is 0 and 0.0 elsewhere (the `confidence` map of
 *   as_disp_to_points_gated as it is).  diff_l, diff_r: fp32 e, the quiet NaN 0x7FC00000 where the code is 3 or 4.
 *   counts: int32 [B][2][5] (image, view 0 = left / 1 = right, code), 4-byte aligned, OVERWRITTEN by the call: cleared by a memset
 *   node, then integer adds only, so exact and independent of the order.  H * W <= 2^31 - 1.
 *
 * as_lr_fill: per row of disp [B][1][H][W] with code uint8 [B][1][H][W]: out = disp where the code is 0; elsewhere, with l the
 *   value of the nearest code-0 pixel to the left in the row and r that of the nearest one to the right, out = (r < l) ? r : l
 *   when both exist (the smaller is the background), the existing one when only one does, and 0.0 ("no measurement") when the
 *   row holds no code-0 pixel.  Selection only.  out may not alias disp.  One workgroup per row; a pass covers 1024 pixels, a
 *   longer row is carried from pass to pass. */
int as_mirror_pair(const float* left, const float* right, int B, int C, int H, int W, float* left_batch, float* right_batch,
                   void* stream);
int as_flip_w(const float* src, int64_t planes, int H, int W, float* dst, void* stream);
int as_lr_check(const float* disp_l, const float* disp_r, int mirrored, int B, int H, int W, float tol_abs, float tol_rel,
                uint8_t* code_l, uint8_t* code_r, float* valid_l, float* valid_r, float* diff_l, float* diff_r, int32_t* counts,
                void* stream);
int as_lr_fill(const float* disp, const uint8_t* code, int B, int H, int W, float* out, void* stream);

/* ---- disparity post-filter: discontinuity (flying-pixel) check and speckle removal (csrc/disp_filter.hip) ----
 * The two steps a classical pipeline runs on a disparity map before it becomes a point cloud; the reference has neither.
 * tests/disp_filter_ref.py restates both contracts in numpy float32.  Conventions as in the block above: dense fp32
 * [B][1][H][W] maps, uint8 codes of the same shape, stream-ordered, nothing allocated, nothing read back (capturable).
 * AS_ERR_ARG before anything is enqueued: a NULL required pointer, a non-positive extent, H * W > 2^31 - 1, B > 65535, a NaN or
 * negative tolerance (+inf is a tolerance), an output that shares a byte with an input or with another output.
 * Codes extend those of as_lr_check: 0 keep, 1-3 as the check defines them, 4 bad input, 5 discontinuity, 6 speckle; as_lr_fill
 * treats every non-zero code as "fill me", so the new ones feed it unchanged.
 * A pixel is USABLE when code_in is NULL or 0 there and its disparity d has d >= 0 and d != +inf (as_lr_check's step 1; -0.0 is
 * usable, a NaN is not).  code_in (optional) is the code map of an earlier stage, e.g. as_lr_check's code_l.
 * counts (optional): int32 [B][7], 4-byte aligned, OVERWRITTEN: cleared by a small launch, then integer adds only; a code above 6
 * passed through from code_in is written to `code` and counted nowhere.  valid: fp32 1.0 where the code is 0, 0.0 elsewhere.
 *
 * as_disp_edge_check: one kernel launch (and the clearing launch).  code, valid, jump, counts are each optional, one is required.
 *   At pixel p with d = disp[p], every fp32 operation rounded once and none contracted:
 *     1  code_in[p] != 0: the code passes through.
 *     2  p not usable otherwise: code 4.
 *     3  tol = fmaxf(tol_abs, tol_rel * d) (a NaN product, inf * 0, leaves tol_abs).  Over the 4-neighbours q (left, right, up,
 *        down) that lie in the image and are usable, e_q = fabsf(d - disp[q]).  Code 5 if any e_q > tol, else 0.  A neighbour
 *        that is not usable is skipped: a pixel beside a hole is not punished for it.  No usable neighbour: code 0.
 *   jump: fp32, the largest e_q, 0.0 without a usable neighbour, the quiet NaN 0x7FC00000 for steps 1 and 2.
 *
 * as_disp_speckle: connected components of the usable pixels and the rejection of the small ones; four kernel launches (three
 *   when H == 1) and the clearing launch.  Two usable 4-neighbours p, q of one image are JOINED iff
 *   fabsf(disp[p] - disp[q]) <= max_diff: one subtraction, the same bits from either side.  max_diff >= 0, +inf joins every usable
 *   pair; 0 <= max_size <= 2^31 - 1, and max_size = 0 rejects nothing.
 *   label (required): int32, the smallest linear index y * W + x of the pixel's component in its image, -1 where not usable.
 *   size  (required): int32, the component's pixel count, 0 where not usable.
 *   code  (optional): code_in where that is non-zero; 4 where the pixel is otherwise not usable; 6 where size <= max_size; else 0.
 *   label and size are also the working arrays (parent links, root counters); every call initialises them itself, so a replay
 *   needs no clear.  The result is a pure function of the input, bit-identical from run to run.  The kernels work on tiles of
 *   4 rows x 256 columns, a wave on 64 consecutive pixels of a row. */
int as_disp_edge_check(const float* disp, const uint8_t* code_in, int B, int H, int W, float tol_abs, float tol_rel, uint8_t* code,
                       float* valid, float* jump, int32_t* counts, void* stream);
int as_disp_speckle(const float* disp, const uint8_t* code_in, int B, int H, int W, float max_diff, int max_size, int32_t* label,
                    int32_t* size, uint8_t* code, float* valid, int32_t* counts, void* stream);

/* ---- edge-aware disparity smoothing: the image-guided weighted median (csrc/disp_smooth.hip) ----
 * The step that REPAIRS a map where the stages above only reject or fill along a row: the weighted median of Ma et al. (ICCV
 * 2013) with integer weights from the guide image; with every weight 1 it is the plain median a classical matcher ends in.  The
 * reference has nothing like it.  tests/disp_smooth_ref.py restates the contract in numpy.  Conventions as in the block above:
 * dense fp32 [B][1][H][W] maps, uint8 codes of the same shape, USABLE as defined there, stream-ordered, nothing allocated, nothing
 * read back (capturable).  One kernel launch (and the clearing launch when counts is given).
 * AS_ERR_ARG before anything is enqueued: NULL disp or out, a non-positive extent, H * W > 2^31 - 1, B > 65535, a guide with C
 * outside {1, 3}, a guide without a table or a table without a guide, radius outside 1 .. 7, fill outside {0, 1}, min_support < 1,
 * disp, guide, weight_lut, out or counts not 4-byte aligned, an output that shares a byte with an input or with another output.
 *
 *   guide       (optional) fp32 [B][C][H][W], C 1 or 3, the network's image planes in [0, 1].  At every pixel and channel
 *               g = (int)rintf(fminf(fmaxf(v, 0.f), 1.f) * 255.f): a NaN becomes 0, one rounding in the product, ties to even.
 *   weight_lut  768 int32 on the device, with a guide only; each entry is clamped to 0 .. 65535 when it is read.
 *               guide == NULL (and weight_lut == NULL): every weight is 1.
 *   weight      of tap q seen from the centre p: w = lut[sum over c of |g_c(p) - g_c(q)|], an integer.
 *   taps        the pixels q of the (2 * radius + 1)^2 window around p that lie in the image (no border replication) and are
 *               usable (code_in NULL or 0 there, disp[q] >= 0 and != +inf).  The centre is a tap like any other if it is usable.
 *               n = their number, Wt = the sum of their weights (at most 225 * 65535).
 *   selection   the taps ordered by the bit pattern of their disparity read as signed int32 (the numeric order of usable
 *               values, -0.0 before +0.0); m(p) = the disparity of the first tap in that order at which
 *               2 * (cumulative weight) >= Wt.  Equal weights and even n: the LOWER median.
 *   per pixel   p usable and Wt > 0: out = m(p).  p usable and Wt == 0: out = disp[p].
 *               p not usable, fill == 1, n >= min_support and Wt > 0: out = m(p), code 0: FILLED.
 *               p not usable otherwise: out = the bits of disp[p] (a NaN keeps its payload); code = code_in[p] where that is
 *               non-zero (codes above 6 included), else 4.
 *   out         (required) fp32; always the bits of one input disparity.
 *   code        (optional) uint8: 0 wherever out holds a kept or a filled value.
 *   counts      (optional) int32 [B][4], OVERWRITTEN: usable and bits unchanged, usable and bits changed, filled, still rejected;
 *               the four sum to H * W per image.
 * The result is a pure function of the inputs, bit-identical from run to run.  The kernel works on tiles of 16 rows x 64 columns. */
int as_disp_wmedian(const float* disp, const uint8_t* code_in, const float* guide, int C, const int32_t* weight_lut, int B, int H,
                    int W, int radius, int fill, int min_support, float* out, uint8_t* code, int32_t* counts, void* stream);

/* ---- stereo rectification of raw camera pairs (csrc/rectify.hip) ----
 * The stage in front of the network for a rig, or a data set, whose images are NOT rectified: undistortion and the rectifying
 * rotation as one bilinear gather per output pixel, what a host pipeline does with cv2.initUndistortRectifyMap + cv2.remap.
 * tests/rectify_ref.py restates the contract in numpy float32.  Stream-ordered, nothing allocated, nothing read back (capturable);
 * the camera structs are HOST pointers read at call time, as as_depth_camera is.
 * AS_ERR_ARG before anything is enqueued: a NULL required pointer, a non-positive extent, C outside {1, 3}, 2 * B > 65535,
 * |i0| or |j0| above 2^30, H * W or H0 * W0 of 2^30 or more, more than 4 * 65535 rows, an output that is not 4-byte aligned.
 *
 * as_rectify_camera: m is inv(K_new[:3,:3] * R_rect) rounded to fp32 ONCE, after an fp64 inversion on the host (row-major): it
 * takes a rectified pixel (u, v, 1) to a ray in the raw camera's frame.  fx, fy, cx, cy are the RAW camera's matrix, k1 .. k6,
 * p1, p2 its distortion coefficients in OpenCV's order (k1, k2, p1, p2, k3, k4, k5, k6); absent ones are 0.
 *
 * (i0, j0, H, W) is the window of the rectified image that is produced; any window, also one that leaves what the raw image
 * covers.  At output pixel (y, x), x in [0, W), y in [0, H), every line single IEEE fp32 operations in the written order, none
 * contracted, every division correctly rounded:
 *     u = (float)(x + j0), v = (float)(y + i0)
 *     X = (m0*u + m1*v) + m2;  Y = (m3*u + m4*v) + m5;  Z = (m6*u + m7*v) + m8
 *     xn = X / Z;  yn = Y / Z;  xx = xn*xn;  yy = yn*yn;  xy = xn*yn;  r2 = xx + yy
 *     num = ((k3*r2 + k2)*r2 + k1)*r2 + 1.f;  den = ((k6*r2 + k5)*r2 + k4)*r2 + 1.f;  rad = num / den
 *     xd = (xn*rad + (2.f*p1)*xy) + p2*(r2 + 2.f*xx)
 *     yd = (yn*rad + p1*(r2 + 2.f*yy)) + (2.f*p2)*xy
 *     us = fx*xd + cx;  vs = fy*yd + cy
 *     valid = Z > 0 && us >= 0 && us <= (float)(W0-1) && vs >= 0 && vs <= (float)(H0-1)          (a NaN fails)
 *   and, for a valid pixel only (the coordinates of an invalid one may be NaN, infinite or beyond int32):
 *     x0 = (int)floorf(us); x1 = min(x0+1, W0-1); ax = us - (float)x0;  y0, y1, ay likewise
 *     per channel, as float: a, b = row y0 at x0, x1;  c, d = row y1 at x0, x1
 *     top = (b-a)*ax + a;  bot = (d-c)*ax + c;  val = (bot-top)*ay + top;  out = val / 255.f
 *   an invalid pixel is `fill` in every plane.
 * Validity depends on the calibration and the window only, never on the image: the per-frame call writes no mask.
 * Not modelled: fisheye lenses; and, as in OpenCV, the forward polynomial is evaluated wherever the ray points, so far outside the
 * field of view a strongly negative radial term folds back into the image (valid, with content from elsewhere).
 *
 * as_rectify_map: one launch.  map_x, map_y (us, vs as computed, NaN included) and valid (1.0f / 0.0f) are each [H][W] fp32 and
 *   each optional; one is required.  Called once when a rectifier is built.
 * as_rectify_pair: one launch for both cameras and the whole batch.  src_l, src_r: [B][H0][W0][C] uint8, C in {1, 3} (the
 *   layout as_decode_rgb8 takes, and mono cameras); dst_l, dst_r: [B][3][H][W] fp32 (C = 1 writes one value to all three planes).
 *   The coordinates are recomputed by the same device function as_rectify_map runs, so its map is exactly what was sampled.
 *   A workgroup covers 4 rows x 256 columns, a lane pixels lane, lane + 64, lane + 128 and lane + 192 of them: one route for
 *   every width and alignment (the outputs need 4-byte alignment only). */
typedef struct as_rectify_camera {
  float m[9];
  float fx, fy, cx, cy;
  float k1, k2, p1, p2, k3, k4, k5, k6;
} as_rectify_camera;
int as_rectify_map(const as_rectify_camera* cam, int H0, int W0, int i0, int j0, int H, int W, float* map_x, float* map_y,
                   float* valid, void* stream);
int as_rectify_pair(const uint8_t* src_l, const uint8_t* src_r, int B, int H0, int W0, int C, const as_rectify_camera* cam_l,
                    const as_rectify_camera* cam_r, int i0, int j0, int H, int W, float fill, float* dst_l, float* dst_r,
                    void* stream);

/* ---- semi-global matching: a network-independent disparity (csrc/sgm.hip) ----
 * The classical matcher beside the network: census transform, Hamming cost, path aggregation (Hirschmueller 2008), winner
 * selection for both views out of one volume.  A baseline to score the network against, and sparse proxy labels once the
 * left-right check and the speckle filter have thinned it.  tests/sgm_ref.py restates the four contracts in numpy; all of it is
 * integer arithmetic up to the sub-pixel division, so every result is exact and independent of any order.  Conventions as in the
 * blocks above: dense fp32 [B][C][H][W] images and [B][1][H][W] maps, stream-ordered, nothing allocated, nothing read back
 * (capturable).  AS_ERR_ARG before anything is enqueued: a NULL required pointer, a non-positive extent, C outside {1, 3},
 * D outside 1 .. 256, paths outside {4, 8}, P1 < 0, P2 < P1 or P2 > 255, uniqueness outside 0 .. 99, B > 65535,
 * H * W * D > 2^31 - 1 (H * W > 2^31 - 1 for the census), a census pointer that is not 8-byte aligned, a workspace pointer that
 * is not 16-byte aligned, an output that shares a byte with an input or with another output.
 *
 * as_sgm_census: one launch.  img [B][C][H][W] fp32 -> census uint64 [B][H][W].  Grey value, each fp32 operation rounded once
 *   and none contracted: C == 3: g = (0.299f * r + 0.587f * g) + 0.114f * b of planes 0, 1, 2; C == 1: the plane itself.
 *   q = (int)floorf(fminf(fmaxf(g * 255.0f + 0.5f, 0.0f), 255.0f)); a NaN gives 0 through fmaxf.  Window 9 wide x 7 high: for
 *   dy in -3 .. 3, dx in -4 .. 4, bit k = (dy + 3) * 9 + (dx + 4) is q[clamp(y + dy)][clamp(x + dx)] < q[y][x], coordinates
 *   clamped to the image.  Bit 31 (the centre) and bit 63 are always 0.  A workgroup covers 8 rows x 32 columns and holds their q
 *   with the halo in LDS.
 *
 * as_sgm_workspace: host function.  Bytes of the aggregation volume S, uint16 [B][H][W][D] with D contiguous, which is all the
 *   kernels need; 0 on bad arguments.  S begins at the workspace pointer; as_sgm_select reads exactly this layout.
 *
 * as_sgm_aggregate: matching cost, never stored: C(y,x,d) = popcount(census_l[y][x] ^ census_r[y][x-d]) for x - d >= 0, and 64
 *   for x - d < 0 (worse than any real cost).  Path cost for a direction r = (dy, dx), p - r the predecessor of p and
 *   m = min_k L_r(p-r, k):
 *     L_r(p,d) = C(p,d) + min( L_r(p-r,d), L_r(p-r,d-1) + P1, L_r(p-r,d+1) + P1, m + P2 ) - m,
 *   the d-1 and d+1 terms absent at the ends of the range, and L_r(p,d) = C(p,d) when p - r lies outside the image.
 *   paths = 4: r in (0,+1), (0,-1), (+1,0), (-1,0); paths = 8: those and the four diagonals (+-1,+-1).
 *   S(p,d) = sum over r of L_r(p,d) <= 8 * (64 + 255) = 2552.  The call initialises S itself: a replay needs no clear.
 *   Launches: one for the two horizontal paths (it writes S = L(0,+1), then adds L(0,-1) on the way back), then one per remaining
 *   direction (read-add-write of S): 3 launches at 4 paths, 7 at 8.  A vertical or diagonal line is walked as a column walk: x
 *   advances by dx per row and wraps modulo W, the recurrence being reset (L = C) at the wrap, so every launch has B * W lines
 *   of H pixels.  A pixel's D disparities lie four to a lane over the smallest power of two of lanes that holds them; the minimum
 *   over D is taken across those lanes in registers.
 *
 * as_sgm_select: one launch (and the clearing launch when counts is given).  Every output is optional, one is required.
 *   Left view at (y,x): the column s[d] = S(y,x,d), d in 0 .. n-1 with n = D.  Right view at (y,x): the column
 *   s[d] = S(y,x+d,d), d in 0 .. n-1 with n = min(D, W - x): the same volume read along its diagonal.
 *     1  d* = the SMALLEST d attaining the minimum, s1 = s[d*].
 *     2  not unique iff some k with |k - d*| > 1 has s[k] * (100 - uniqueness) < s1 * 100 (int32; uniqueness 0 rejects nothing).
 *     3  if 0 < d* < n-1 and den = 2 * (s[d*-1] + s[d*+1] - 2 * s1) > 0 (integers):
 *        value = (float)d* + (float)(s[d*-1] - s[d*+1]) / (float)den, one correctly rounded division and one sum;
 *        otherwise value = (float)d*.
 *     4  code (uint8, extending as_disp_speckle's table by one): 3 out of view, left view only, when d* > x; else 7 not unique;
 *        else 0.
 *     5  disp = value where the code is 0, `fill` (passed through bit for bit) elsewhere.
 *   counts: int32 [B][2][8] (image, view 0 = left / 1 = right, code), 4-byte aligned, OVERWRITTEN: cleared by a small launch,
 *   then integer adds only. */
int as_sgm_census(const float* img, int B, int C, int H, int W, uint64_t* census, void* stream);
int64_t as_sgm_workspace(int B, int H, int W, int D);
int as_sgm_aggregate(const uint64_t* census_l, const uint64_t* census_r, int B, int H, int W, int D, int P1, int P2, int paths,
                     void* workspace, void* stream);
int as_sgm_select(const void* workspace, int B, int H, int W, int D, int uniqueness, float fill, float* disp_l, uint8_t* code_l,
                  float* disp_r, uint8_t* code_r, int32_t* counts, void* stream);

/* ---- measurement hook (bench.py roofline leg) -----------------------------------
 * When enabled, as_conv32_fwd and as_conv32_wgrad bracket their main kernel with HIP events on the
 * launch stream and account its algorithmic FLOPs (2 * voxels * 32 * 32 * taps).  Kernel ids:
 * 0 conv32_fwd_kernel<taps> (direct-load forward/dgrad), 1 conv32_wgrad_kernel<..> (direct-load wgrad),
 * 2 conv32_lds_kernel (LDS-staged 3x3 forward/dgrad), 3 conv32_wgrad_lds_kernel.
 * HBM-bound passes account algorithmic BYTES in the same slot: 4 as_bn_act_fwd (2 or 3 tensors x interior
 * bytes), 5 as_bn_act_bwd (its kernels together: 5 tensor passes, fewer when stages are fused elsewhere).
 * 6 conv32_lds_kernel<3,*> (the data gradient that also carries stage 1 of the next BatchNorm backward); id 2 then
 * counts the other flavours only.
 * as_prof_read synchronises on the recorded events.
 * Disabled by default; must stay disabled under hipGraph capture. */
int as_prof_enable(int on);
int as_prof_reset(void);
int as_prof_read(int kernel_id, int64_t* launches, double* total_ms, double* total_flops);

#ifdef __cplusplus
}
#endif
#endif  /* ADAPTIVE_STEREO_HIP_H_ */
