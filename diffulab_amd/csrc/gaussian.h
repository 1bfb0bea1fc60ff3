// Device helpers of Gaussian diffusion that the sampler steps (sampler.hip) and the loss heads (loss.hip) share.
#pragma once
#include "common.h"

__device__ __forceinline__ float x_start_from(int mean_type, float out, float xt, float sab, float ab, float c1,
                                              float c2) {
  if (mean_type == DL_MEAN_XSTART) return out;
  if (mean_type == DL_MEAN_EPSILON) return (1.0f / sab) * xt - (sqrtf(1.0f - ab) / sab) * out;  // ddpm.py:118-121
  if (mean_type == DL_MEAN_V) return sab * xt - sqrtf(1.0f - ab) * out;  // Salimans & Ho (2022): v = sab eps - sqrt(1 - ab) x0
  return (1.0f / c1) * out - (c2 / c1) * xt;                                                    // ddpm.py:99-102
}
// dynamic thresholding (Saharia et al., Imagen, 2022): x0 clamped to the sample's own threshold s >= 1 and divided by it
__device__ __forceinline__ float threshold_x0(float x0, float s) { return fminf(fmaxf(x0, -s), s) / s; }
// learned variances (ddpm.py:212-222, 268-282): pred / pu are [B, 2 chw], element (b, r) has its mean output at b 2chw + r and its raw
// variance output at b 2chw + chw + r, both read in place.  tab: f32 [6][T] = sqrt_ab, ab, coef1, coef2, posterior_log_variance_clipped,
// betas.  The log-variance of one element, shared with the hybrid loss:
__device__ __forceinline__ float learned_log_var(int var_mode, float v, float min_log, float beta) {
  if (var_mode == DL_VAR_LEARNED) return v;
  const float w = (v + 1.0f) / 2.0f;  // ddpm.py:218-221; log(betas[t]) in f32 after the gather
  return w * logf(beta) + (1.0f - w) * min_log;
}
