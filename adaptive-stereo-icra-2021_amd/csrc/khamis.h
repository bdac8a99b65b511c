// The Khamis robust loss per pixel (reference utils/loss_functions.py:15), one definition for the three files that form it:
// photometric.hip (as_khamis_fwd/bwd), supervised.hip (as_khamis2_fwd/bwd) and proxy_loss.hip (as_proxy_term_fwd/bwd).
// How khamis_slope rounds follows the file that includes this header: photometric.hip and proxy_loss.hip include it below their
// `#pragma clang fp contract(off)` (d * d and + 4 round separately, IEEE division and square root: as_proxy_term_bwd is bit for bit
// as_khamis_bwd), supervised.hip includes it under the compiler's default (d * d + 4 is one fused operation there, as it always
// was).  Each file's results are what they were before the definition was shared.
#pragma once
#include "as_common.h"

// workgroups of the two-stage fp64 sums of as_masked_sum, as_khamis_fwd and as_proxy_term_fwd: min(ceil(n / 256), MS_BLOCKS)
#define MS_BLOCKS 512

// sqrt((g - p)^2 + 4) / 2 - 1 in fp32.  The _rn intrinsics do not keep the operations apart: HIP defines them as plain operators
// in its own header, which no pragma of the including file reaches, so in all three files this compiles to fma(d, d, 4), the
// hardware's square root (v_sqrt_f32, within an ulp of the root, no correction step), fma(s, 0.5, -1): three roundings, the
// same bits in every file.  A host restatement that rounds every operation agrees to two ulps of the value + 1 per pixel
// (tests/proxy_loss_ref.py).
__device__ inline float khamis_value(float g, float p) {
  const float d = g - p;
  return __fsub_rn(__fdiv_rn(__fsqrt_rn(__fadd_rn(__fmul_rn(d, d), 4.f)), 2.f), 1.f);
}
// scale * d value / d p = -scale * (g - p) / (2 sqrt((g - p)^2 + 4))
__device__ inline float khamis_slope(float g, float p, float scale) {
  const float d = g - p;
  return -scale * d / (2.f * sqrtf(d * d + 4.f));
}
