// HBM-bound kernels of sampling: the sampler steps, CFG rescale, the quantile / dynamic threshold, the inpainting blend.
// The steps are grid-stride loops (cdna_hip_programming.md Appendix B "Element-wise").
#include "common.h"
#include "gaussian.h"

// ---------------------------------------------------------------- sampler steps
// GD (the _g entry points, guided sampling): `mul` f32 [B] scales the combined prediction of sample i / chw (CFG rescale, Lin et al.
// 2023), `thr` f32 [B] is the sample's dynamic threshold (Saharia et al. 2022; the Gaussian kernels only).  Either may be NULL.  The
// GD = false instantiations are what the entry points without _g launch: they read neither array and carry no branch on them.
// The arrays travel in the kernel's last argument, a struct that for GD = false holds exactly what that argument was before (n for the
// flow kernels, chw for the Gaussian ones): the same bytes at the same kernarg offsets, so the plain entry points keep their code.
template <bool GD>
struct FlowTail {
  int64_t n;
};
template <>
struct FlowTail<true> {
  int64_t n;
  const float* mul;
  int64_t chw;
};
template <bool GD>
struct GaussTail {
  int64_t chw;
};
template <>
struct GaussTail<true> {
  int64_t chw;
  const float *mul, *thr;
};
template <bool GD>
__global__ void euler_step_k(const float* __restrict__ x, const float* __restrict__ v, const float* __restrict__ vu,
                             float g, float t_curr, float dt, float* __restrict__ xp, float* __restrict__ x0,
                             const FlowTail<GD> tail) {
  const int64_t n = tail.n;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    float vv = v[i];
    if (vu) {
      const float u = vu[i];
      vv = u + g * (vv - u);
    }
    if constexpr (GD) {
      if (tail.mul) vv *= tail.mul[i / tail.chw];
    }
    const float xi = x[i];
    xp[i] = xi - vv * dt;
    if (x0) x0[i] = xi - vv * t_curr;
  }
}
static int euler_launch(const float* x, const float* v, const float* v_uncond, float guidance, const float* cfg_mul, float t_curr,
                        float dt, float* x_prev, float* x0_est, int64_t n, int64_t chw, dl_stream_t stream) {
  if (cfg_mul)
    hipLaunchKernelGGL(euler_step_k<true>, ew_grid(n), 256, 0, (hipStream_t)stream, x, v, v_uncond, guidance, t_curr, dt, x_prev,
                       x0_est, FlowTail<true>{n, cfg_mul, chw});
  else
    hipLaunchKernelGGL(euler_step_k<false>, ew_grid(n), 256, 0, (hipStream_t)stream, x, v, v_uncond, guidance, t_curr, dt, x_prev,
                       x0_est, FlowTail<false>{n});
  DL_LAUNCH_CHECK();
  return DL_OK;
}
extern "C" int dl_euler_step(const float* x, const float* v, const float* v_uncond, float guidance, float t_curr,
                             float dt, float* x_prev, float* x0_est, int64_t n, dl_stream_t stream) {
  DL_CHECK_ARG(x && v && x_prev && n > 0, "dl_euler_step: bad args");
  return euler_launch(x, v, v_uncond, guidance, nullptr, t_curr, dt, x_prev, x0_est, n, 0, stream);
}
extern "C" int dl_euler_step_g(const float* x, const float* v, const float* v_uncond, float guidance, const float* cfg_mul,
                               float t_curr, float dt, float* x_prev, float* x0_est, int64_t batch, int64_t chw,
                               dl_stream_t stream) {
  DL_CHECK_ARG(x && v && x_prev && batch > 0 && chw > 0, "dl_euler_step_g: bad args");
  return euler_launch(x, v, v_uncond, guidance, cfg_mul, t_curr, dt, x_prev, x0_est, batch * chw, chw, stream);
}

// variable-step Adams-Bashforth 2 on v in t (this project's).  HIST false is euler_step_k's body, expression for expression, plus the
// store of the combined v that the next step reads as its history.
template <bool GD, bool HIST>
__global__ void ab2_step_k(const float* __restrict__ x, const float* __restrict__ v, const float* __restrict__ vu,
                           const float* __restrict__ vl, float g, float t_curr, float dt, float w, float* __restrict__ xp,
                           float* __restrict__ x0, float* __restrict__ vo, const FlowTail<GD> tail) {
  const int64_t n = tail.n;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    float vv = v[i];
    if (vu) {
      const float u = vu[i];
      vv = u + g * (vv - u);
    }
    if constexpr (GD) {
      if (tail.mul) vv *= tail.mul[i / tail.chw];
    }
    const float xi = x[i];
    if constexpr (HIST) {
      const float d = (1.0f + w) * vv - w * vl[i];
      xp[i] = xi - d * dt;
    } else {
      xp[i] = xi - vv * dt;
    }
    if (x0) x0[i] = xi - vv * t_curr;
    vo[i] = vv;
  }
}
extern "C" int dl_ab2_step(const float* x, const float* v, const float* v_uncond, float guidance, const float* cfg_mul,
                           const float* v_last, float t_curr, float dt, float w, float* x_prev, float* x0_est, float* v_out,
                           int64_t batch, int64_t chw, dl_stream_t stream) {
  DL_CHECK_ARG(x && v && x_prev && v_out && batch > 0 && chw > 0, "dl_ab2_step: bad args");
  DL_CHECK_ARG(v_out != v && v_out != v_uncond && v_out != v_last && v_out != x, "dl_ab2_step: v_out aliases an input");
  DL_CHECK_ARG(!v_last || (w == w && w - w == 0.0f), "dl_ab2_step: w %g is not finite", (double)w);
  const int64_t n = batch * chw;
  const FlowTail<true> on{n, cfg_mul, chw};
  const FlowTail<false> off{n};
#define AB2(G, H, TAIL)                                                                                                          \
  hipLaunchKernelGGL((ab2_step_k<G, H>), ew_grid(n), 256, 0, (hipStream_t)stream, x, v, v_uncond, v_last, guidance, t_curr, dt, w, \
                     x_prev, x0_est, v_out, TAIL)
  if (v_last) {
    if (cfg_mul) AB2(true, true, on); else AB2(false, true, off);
  } else {
    if (cfg_mul) AB2(true, false, on); else AB2(false, false, off);
  }
#undef AB2
  DL_LAUNCH_CHECK();
  return DL_OK;
}

template <bool GD>
__global__ void em_step_k(const float* __restrict__ x, const float* __restrict__ v, const float* __restrict__ vu,
                          float g, const float* __restrict__ noise, const float* __restrict__ xpin, float t_curr,
                          float dt, float drift_c, float std, float log_std, float* __restrict__ xp,
                          float* __restrict__ mean, float* __restrict__ x0, float* __restrict__ lp,
                          const FlowTail<GD> tail) {
  const int64_t n = tail.n;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const float half_log_2pi = 0.91893853320467274178f;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    float vv = v[i];
    if (vu) {
      const float u = vu[i];
      vv = u + g * (vv - u);
    }
    if constexpr (GD) {
      if (tail.mul) vv *= tail.mul[i / tail.chw];
    }
    const float xi = x[i];
    // x - (v + sigma^2/(2t) (x + (1-t) v)) dt
    const float m = xi - (vv + drift_c * (xi + (1.0f - t_curr) * vv)) * dt;
    const float xpv = xpin ? xpin[i] : (m + std * noise[i]);
    xp[i] = xpv;
    if (mean) mean[i] = m;
    if (x0) x0[i] = xi - vv * t_curr;
    if (lp) {
      const float d = xpv - m;
      lp[i] = -(d * d / (2.0f * std * std) + log_std + half_log_2pi);
    }
  }
}
static int em_launch(const float* x, const float* v, const float* v_uncond, float guidance, const float* cfg_mul, const float* noise,
                     const float* x_prev_in, float t_curr, float dt, float sigma, float std, float* x_prev, float* mean,
                     float* x0_est, float* logprob, int64_t n, int64_t chw, dl_stream_t stream) {
  const float drift_c = (float)((double)sigma * (double)sigma / (2.0 * (double)t_curr));
  if (cfg_mul)
    hipLaunchKernelGGL(em_step_k<true>, ew_grid(n), 256, 0, (hipStream_t)stream, x, v, v_uncond, guidance, noise, x_prev_in, t_curr,
                       dt, drift_c, std, logf(std), x_prev, mean, x0_est, logprob, FlowTail<true>{n, cfg_mul, chw});
  else
    hipLaunchKernelGGL(em_step_k<false>, ew_grid(n), 256, 0, (hipStream_t)stream, x, v, v_uncond, guidance, noise, x_prev_in, t_curr,
                       dt, drift_c, std, logf(std), x_prev, mean, x0_est, logprob, FlowTail<false>{n});
  DL_LAUNCH_CHECK();
  return DL_OK;
}
extern "C" int dl_euler_maruyama_step(const float* x, const float* v, const float* v_uncond, float guidance,
                                      const float* noise, const float* x_prev_in, float t_curr, float dt,
                                      float sigma, float std, float* x_prev, float* mean, float* x0_est,
                                      float* logprob, int64_t n, dl_stream_t stream) {
  DL_CHECK_ARG(x && v && x_prev && n > 0, "dl_euler_maruyama_step: bad args");
  DL_CHECK_ARG((noise != nullptr) != (x_prev_in != nullptr), "dl_euler_maruyama_step: exactly one of noise/x_prev_in");
  return em_launch(x, v, v_uncond, guidance, nullptr, noise, x_prev_in, t_curr, dt, sigma, std, x_prev, mean, x0_est, logprob, n, 0,
                   stream);
}
extern "C" int dl_euler_maruyama_step_g(const float* x, const float* v, const float* v_uncond, float guidance,
                                        const float* cfg_mul, const float* noise, const float* x_prev_in, float t_curr, float dt,
                                        float sigma, float std, float* x_prev, float* mean, float* x0_est, float* logprob,
                                        int64_t batch, int64_t chw, dl_stream_t stream) {
  DL_CHECK_ARG(x && v && x_prev && batch > 0 && chw > 0, "dl_euler_maruyama_step_g: bad args");
  DL_CHECK_ARG((noise != nullptr) != (x_prev_in != nullptr), "dl_euler_maruyama_step_g: exactly one of noise/x_prev_in");
  return em_launch(x, v, v_uncond, guidance, cfg_mul, noise, x_prev_in, t_curr, dt, sigma, std, x_prev, mean, x0_est, logprob,
                   batch * chw, chw, stream);
}

// LV false: pred / pu are [B, chw], rows 4 and 5 of tab are the variance and its log (var_mode is not read).  LV true: as above.
template <bool LV, bool GD>
__global__ void ddpm_step_k(const float* __restrict__ pred, const float* __restrict__ pu, float g,
                            const float* __restrict__ xt, const float* __restrict__ noise,
                            const int32_t* __restrict__ t, const float* __restrict__ tab, int32_t T, int mean_type,
                            int clamp_x, int var_mode, float* __restrict__ xp, float* __restrict__ x0o,
                            float* __restrict__ mo, float* __restrict__ so, float* __restrict__ lp, int64_t n,
                            const GaussTail<GD> tail) {
  const int64_t chw = tail.chw;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const int64_t b = i / chw;
    const int32_t ti = t[b];
    const float sab = tab[ti], ab = tab[T + ti], c1 = tab[2 * T + ti], c2 = tab[3 * T + ti];
    const float r4 = tab[4 * T + ti], r5 = tab[5 * T + ti];  // LV: min_log, beta; else var, lv
    const int64_t pi = LV ? i + b * chw : i;
    float o = pred[pi], v = 0.0f;
    if constexpr (LV) v = pred[pi + chw];
    if (pu) {  // LV: the CFG combine acts on the whole 2C tensor before the chunk (gaussian_diffusion.py:253-255)
      const float uo = pu[pi];
      o = uo + g * (o - uo);
      if constexpr (LV) {
        const float uv = pu[pi + chw];
        v = uv + g * (v - uv);
      }
    }
    if constexpr (GD) {  // the mean half only: the variance half keeps the plain combine
      if (tail.mul) o *= tail.mul[b];
    }
    float lv = r5, var = r4;
    if constexpr (LV) {
      lv = learned_log_var(var_mode, v, r4, r5);
      var = expf(lv);
    }
    const float x = xt[i];
    float x0 = x_start_from(mean_type, o, x, sab, ab, c1, c2);
    if constexpr (GD) {
      if (tail.thr) x0 = threshold_x0(x0, tail.thr[b]);
    }
    if (clamp_x) x0 = fminf(fmaxf(x0, -1.0f), 1.0f);
    const float m = c1 * x0 + c2 * x;
    const float mask = ti > 0 ? 1.0f : 0.0f;
    const float xpv = m + mask * noise[i] * expf(0.5f * lv);
    xp[i] = xpv;
    if (x0o) x0o[i] = x0;
    if (mo) mo[i] = m;
    const float vs = fmaxf(var, 1e-20f);
    if (so) so[i] = sqrtf(vs);
    if (lp) {
      const float d = xpv - m;
      lp[i] = (-(d * d) / (2.0f * vs) - logf(6.283185307179586f * vs) * 0.5f) * mask;
    }
  }
}

// x0 of element i as the DDIM-family steps form it: CFG combine, cfg_mul, x_start_from, x0_thr, clamp_x, in that order (the same f32
// expression X0Key evaluates for dl_x0_threshold).  Shared by ddim_step_k and dpmpp_2m_step_k.
// HALVES: pred / pu are [B, 2 chw] and the step reads the mean half in place (learned variances, which DDIM discards: ddim.py:89)
template <bool HALVES, bool GD>
__device__ __forceinline__ float ddim_x0(int64_t i, int64_t chw, const float* __restrict__ pred, const float* __restrict__ pu, float g,
                                         float x, int mean_type, float sab, float ab, float c1, float c2, int clamp_x,
                                         const GaussTail<GD>& tail) {
  const int64_t pi = HALVES ? i + (i / chw) * chw : i;
  float o = pred[pi];
  if (pu) {
    const float u = pu[pi];
    o = u + g * (o - u);
  }
  if constexpr (GD) {
    if (tail.mul) o *= tail.mul[i / chw];
  }
  float x0 = x_start_from(mean_type, o, x, sab, ab, c1, c2);
  if constexpr (GD) {
    if (tail.thr) x0 = threshold_x0(x0, tail.thr[i / chw]);
  }
  if (clamp_x) x0 = fminf(fmaxf(x0, -1.0f), 1.0f);
  return x0;
}
template <bool HALVES, bool GD>
__global__ void ddim_step_k(const float* __restrict__ pred, const float* __restrict__ pu, float g,
                            const float* __restrict__ xt, const float* __restrict__ noise,
                            const int32_t* __restrict__ t, const float* __restrict__ tab, int32_t T, int mean_type,
                            const float* __restrict__ coefs, int clamp_x, float eta, float* __restrict__ xp,
                            float* __restrict__ x0o, float* __restrict__ mo, float* __restrict__ so,
                            float* __restrict__ lp, int64_t n, const GaussTail<GD> tail) {
  const int64_t chw = tail.chw;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const float half_log_2pi = 0.91893853320467274178f;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const int32_t ti = t[i / chw];
    const float sab = tab[ti], ab = tab[T + ti], abp = tab[2 * T + ti];
    const float c1 = coefs ? coefs[ti] : 1.0f, c2 = coefs ? coefs[T + ti] : 0.0f;
    const float x = xt[i];
    const float x0 = ddim_x0<HALVES, GD>(i, chw, pred, pu, g, x, mean_type, sab, ab, c1, c2, clamp_x, tail);
    const float eps = ((1.0f / sab) * x - x0) / sqrtf(1.0f / ab - 1.0f);  // ddpm.py:324-326
    const float sigma = eta * sqrtf((1.0f - abp) / (1.0f - ab)) * sqrtf(1.0f - ab / abp);
    const float m = x0 * sqrtf(abp) + sqrtf(1.0f - abp - sigma * sigma) * eps;
    const float mask = ti > 0 ? 1.0f : 0.0f;
    const float xpv = m + mask * sigma * noise[i];
    xp[i] = xpv;
    if (x0o) x0o[i] = x0;
    if (mo) mo[i] = m;
    if (so) so[i] = sigma;
    if (lp) {
      const float d = xpv - m;
      lp[i] = -(d * d / (2.0f * sigma * sigma) + logf(sigma) + half_log_2pi);
    }
  }
}

// The four entry points of each Gaussian sampler differ in what they accept, not in what they launch.  The plain one takes the
// reference's three mean types and a [B, chw] prediction; _lv the same mean types and the [B, 2 chw] prediction of a learned-variance
// model; _v is v-prediction (Salimans & Ho 2022: x_start_from's DL_MEAN_V case) for either kind of prediction; _g takes every
// mean_type and var_mode, plus the two per-sample arrays of guided sampling.  Each checks its own arguments under its own name, then
// the launcher picks the instantiation from (var_mode, cfg_mul || x0_thr): with both arrays NULL that is the GD = false kernel.
static int gauss_step_check(const char* who, const void* pred, const void* xt, const void* noise, const void* t, const void* tables,
                            const void* x_prev, int32_t T, int mean_type, int mean_max, int var_mode, int var_lo, int var_hi,
                            int64_t batch, int64_t chw) {
  DL_CHECK_ARG(pred && xt && noise && t && tables && x_prev && batch > 0 && chw > 0 && T > 0, "%s: bad args", who);
  DL_CHECK_ARG(mean_type >= DL_MEAN_EPSILON && mean_type <= mean_max, "%s: mean_type %d", who, mean_type);
  DL_CHECK_ARG(var_mode >= var_lo && var_mode <= var_hi, "%s: var_mode %d", who, var_mode);
  return DL_OK;
}
static int ddpm_launch(const float* pred, const float* pred_uncond, float guidance, const float* cfg_mul, const float* x0_thr,
                       const float* xt, const float* noise, const int32_t* t, const float* tables, int32_t T, int mean_type,
                       int var_mode, int clamp_x, float* x_prev, float* x0_est, float* mean, float* std, float* logprob, int64_t batch,
                       int64_t chw, dl_stream_t stream) {
  const int64_t n = batch * chw;
  const GaussTail<true> on{chw, cfg_mul, x0_thr};
  const GaussTail<false> off{chw};
#define DDPM(LV, G, TAIL)                                                                                                            \
  hipLaunchKernelGGL((ddpm_step_k<LV, G>), ew_grid(n), 256, 0, (hipStream_t)stream, pred, pred_uncond, guidance, xt, noise, t, tables, \
                     T, mean_type, clamp_x, var_mode, x_prev, x0_est, mean, std, logprob, n, TAIL)
  if (var_mode == DL_VAR_FIXED) {
    if (cfg_mul || x0_thr) DDPM(false, true, on); else DDPM(false, false, off);
  } else {
    if (cfg_mul || x0_thr) DDPM(true, true, on); else DDPM(true, false, off);
  }
#undef DDPM
  DL_LAUNCH_CHECK();
  return DL_OK;
}
static int ddim_launch(const float* pred, const float* pred_uncond, float guidance, const float* cfg_mul, const float* x0_thr,
                       const float* xt, const float* noise, const int32_t* t, const float* tables, int32_t T, int mean_type,
                       int var_mode, const float* ddpm_coefs, int clamp_x, float eta, float* x_prev, float* x0_est, float* mean,
                       float* std, float* logprob, int64_t batch, int64_t chw, dl_stream_t stream) {
  const int64_t n = batch * chw;
  const GaussTail<true> on{chw, cfg_mul, x0_thr};
  const GaussTail<false> off{chw};
#define DDIM(H, G, TAIL)                                                                                                              \
  hipLaunchKernelGGL((ddim_step_k<H, G>), ew_grid(n), 256, 0, (hipStream_t)stream, pred, pred_uncond, guidance, xt, noise, t, tables, \
                     T, mean_type, ddpm_coefs, clamp_x, eta, x_prev, x0_est, mean, std, logprob, n, TAIL)
  if (var_mode == DL_VAR_FIXED) {
    if (cfg_mul || x0_thr) DDIM(false, true, on); else DDIM(false, false, off);
  } else {
    if (cfg_mul || x0_thr) DDIM(true, true, on); else DDIM(true, false, off);
  }
#undef DDIM
  DL_LAUNCH_CHECK();
  return DL_OK;
}
extern "C" int dl_ddpm_step(const float* pred, const float* pred_uncond, float guidance, const float* xt,
                            const float* noise, const int32_t* t, const float* tables, int32_t T, int mean_type,
                            int clamp_x, float* x_prev, float* x0_est, float* mean, float* std, float* logprob,
                            int64_t batch, int64_t chw, dl_stream_t stream) {
  if (int rc = gauss_step_check("dl_ddpm_step", pred, xt, noise, t, tables, x_prev, T, mean_type, DL_MEAN_XPREV, DL_VAR_FIXED,
                                DL_VAR_FIXED, DL_VAR_FIXED, batch, chw))
    return rc;
  return ddpm_launch(pred, pred_uncond, guidance, nullptr, nullptr, xt, noise, t, tables, T, mean_type, DL_VAR_FIXED, clamp_x, x_prev,
                     x0_est, mean, std, logprob, batch, chw, stream);
}
extern "C" int dl_ddpm_step_lv(const float* pred, const float* pred_uncond, float guidance, const float* xt,
                               const float* noise, const int32_t* t, const float* tables, int32_t T, int mean_type,
                               int var_mode, int clamp_x, float* x_prev, float* x0_est, float* mean, float* std,
                               float* logprob, int64_t batch, int64_t chw, dl_stream_t stream) {
  if (int rc = gauss_step_check("dl_ddpm_step_lv", pred, xt, noise, t, tables, x_prev, T, mean_type, DL_MEAN_XPREV, var_mode,
                                DL_VAR_LEARNED, DL_VAR_LEARNED_RANGE, batch, chw))
    return rc;
  return ddpm_launch(pred, pred_uncond, guidance, nullptr, nullptr, xt, noise, t, tables, T, mean_type, var_mode, clamp_x, x_prev,
                     x0_est, mean, std, logprob, batch, chw, stream);
}
extern "C" int dl_ddpm_step_v(const float* pred, const float* pred_uncond, float guidance, const float* xt, const float* noise,
                              const int32_t* t, const float* tables, int32_t T, int var_mode, int clamp_x, float* x_prev,
                              float* x0_est, float* mean, float* std, float* logprob, int64_t batch, int64_t chw,
                              dl_stream_t stream) {
  if (int rc = gauss_step_check("dl_ddpm_step_v", pred, xt, noise, t, tables, x_prev, T, DL_MEAN_V, DL_MEAN_V, var_mode, DL_VAR_FIXED,
                                DL_VAR_LEARNED_RANGE, batch, chw))
    return rc;
  return ddpm_launch(pred, pred_uncond, guidance, nullptr, nullptr, xt, noise, t, tables, T, DL_MEAN_V, var_mode, clamp_x, x_prev,
                     x0_est, mean, std, logprob, batch, chw, stream);
}
extern "C" int dl_ddpm_step_g(const float* pred, const float* pred_uncond, float guidance, const float* cfg_mul, const float* x0_thr,
                              const float* xt, const float* noise, const int32_t* t, const float* tables, int32_t T, int mean_type,
                              int var_mode, int clamp_x, float* x_prev, float* x0_est, float* mean, float* std, float* logprob,
                              int64_t batch, int64_t chw, dl_stream_t stream) {
  if (int rc = gauss_step_check("dl_ddpm_step_g", pred, xt, noise, t, tables, x_prev, T, mean_type, DL_MEAN_V, var_mode, DL_VAR_FIXED,
                                DL_VAR_LEARNED_RANGE, batch, chw))
    return rc;
  return ddpm_launch(pred, pred_uncond, guidance, cfg_mul, x0_thr, xt, noise, t, tables, T, mean_type, var_mode, clamp_x, x_prev,
                     x0_est, mean, std, logprob, batch, chw, stream);
}
extern "C" int dl_ddim_step(const float* pred, const float* pred_uncond, float guidance, const float* xt,
                            const float* noise, const int32_t* t, const float* tables, int32_t T, int mean_type,
                            const float* ddpm_coefs, int clamp_x, float eta, float* x_prev, float* x0_est,
                            float* mean, float* std, float* logprob, int64_t batch, int64_t chw,
                            dl_stream_t stream) {
  if (int rc = gauss_step_check("dl_ddim_step", pred, xt, noise, t, tables, x_prev, T, mean_type, DL_MEAN_XPREV, DL_VAR_FIXED,
                                DL_VAR_FIXED, DL_VAR_FIXED, batch, chw))
    return rc;
  DL_CHECK_ARG(mean_type != DL_MEAN_XPREV || ddpm_coefs, "dl_ddim_step: xprev needs ddpm_coefs");
  return ddim_launch(pred, pred_uncond, guidance, nullptr, nullptr, xt, noise, t, tables, T, mean_type, DL_VAR_FIXED, ddpm_coefs,
                     clamp_x, eta, x_prev, x0_est, mean, std, logprob, batch, chw, stream);
}
// (DDIM discards the learned variances, ddim.py:89, so _lv takes no var_mode: any learned one reads the mean half in place)
extern "C" int dl_ddim_step_lv(const float* pred, const float* pred_uncond, float guidance, const float* xt,
                               const float* noise, const int32_t* t, const float* tables, int32_t T, int mean_type,
                               const float* ddpm_coefs, int clamp_x, float eta, float* x_prev, float* x0_est,
                               float* mean, float* std, float* logprob, int64_t batch, int64_t chw,
                               dl_stream_t stream) {
  if (int rc = gauss_step_check("dl_ddim_step_lv", pred, xt, noise, t, tables, x_prev, T, mean_type, DL_MEAN_XPREV, DL_VAR_LEARNED,
                                DL_VAR_LEARNED, DL_VAR_LEARNED, batch, chw))
    return rc;
  DL_CHECK_ARG(mean_type != DL_MEAN_XPREV || ddpm_coefs, "dl_ddim_step_lv: xprev needs ddpm_coefs");
  return ddim_launch(pred, pred_uncond, guidance, nullptr, nullptr, xt, noise, t, tables, T, mean_type, DL_VAR_LEARNED, ddpm_coefs,
                     clamp_x, eta, x_prev, x0_est, mean, std, logprob, batch, chw, stream);
}
extern "C" int dl_ddim_step_v(const float* pred, const float* pred_uncond, float guidance, const float* xt, const float* noise,
                              const int32_t* t, const float* tables, int32_t T, int var_mode, int clamp_x, float eta,
                              float* x_prev, float* x0_est, float* mean, float* std, float* logprob, int64_t batch, int64_t chw,
                              dl_stream_t stream) {
  if (int rc = gauss_step_check("dl_ddim_step_v", pred, xt, noise, t, tables, x_prev, T, DL_MEAN_V, DL_MEAN_V, var_mode, DL_VAR_FIXED,
                                DL_VAR_LEARNED_RANGE, batch, chw))
    return rc;
  // (no ddpm_coefs: the posterior-mean coefficients serve DL_MEAN_XPREV only)
  return ddim_launch(pred, pred_uncond, guidance, nullptr, nullptr, xt, noise, t, tables, T, DL_MEAN_V, var_mode, nullptr, clamp_x, eta,
                     x_prev, x0_est, mean, std, logprob, batch, chw, stream);
}
extern "C" int dl_ddim_step_g(const float* pred, const float* pred_uncond, float guidance, const float* cfg_mul, const float* x0_thr,
                              const float* xt, const float* noise, const int32_t* t, const float* tables, int32_t T, int mean_type,
                              int var_mode, const float* ddpm_coefs, int clamp_x, float eta, float* x_prev, float* x0_est,
                              float* mean, float* std, float* logprob, int64_t batch, int64_t chw, dl_stream_t stream) {
  if (int rc = gauss_step_check("dl_ddim_step_g", pred, xt, noise, t, tables, x_prev, T, mean_type, DL_MEAN_V, var_mode, DL_VAR_FIXED,
                                DL_VAR_LEARNED_RANGE, batch, chw))
    return rc;
  DL_CHECK_ARG(mean_type != DL_MEAN_XPREV || ddpm_coefs, "dl_ddim_step_g: xprev needs ddpm_coefs");
  return ddim_launch(pred, pred_uncond, guidance, cfg_mul, x0_thr, xt, noise, t, tables, T, mean_type, var_mode, ddpm_coefs, clamp_x,
                     eta, x_prev, x0_est, mean, std, logprob, batch, chw, stream);
}

// DPM-Solver++(2M) (Lu et al. 2022) in the data-prediction form: x_prev = a x_t + b x0_t + c x0_last, the three coefficients formed
// on the host in fp64 (first or second order, see the header).  x0_t is ddim_x0, so dl_x0_threshold on the same arguments thresholds
// the x0 this step uses.  A zero a drops its term (the final step: x_prev is x0_t bit for bit, whatever x_t holds); HIST false reads
// no x0_last.
template <bool HALVES, bool GD, bool HIST>
__global__ void dpmpp_2m_step_k(const float* __restrict__ pred, const float* __restrict__ pu, float g,
                                const float* __restrict__ xt, const float* __restrict__ xl, const int32_t* __restrict__ t,
                                const float* __restrict__ tab, int32_t T, int mean_type, int clamp_x, float a, float b, float c,
                                float* __restrict__ xp, float* __restrict__ x0o, int64_t n, const GaussTail<GD> tail) {
  const int64_t chw = tail.chw;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const int32_t ti = t[i / chw];
    const float sab = tab[ti], ab = tab[T + ti];
    const float x = xt[i];
    const float x0 = ddim_x0<HALVES, GD>(i, chw, pred, pu, g, x, mean_type, sab, ab, 1.0f, 0.0f, clamp_x, tail);
    float r = b * x0;
    if (a != 0.0f) r += a * x;
    if constexpr (HIST) r += c * xl[i];
    xp[i] = r;
    x0o[i] = x0;
  }
}
extern "C" int dl_dpmpp_2m_step(const float* pred, const float* pred_uncond, float guidance, const float* cfg_mul, const float* x0_thr,
                                const float* xt, const float* x0_last, const int32_t* t, const float* tables, int32_t T, int mean_type,
                                int var_mode, int clamp_x, float a, float b, float c, float* x_prev, float* x0_est, int64_t batch,
                                int64_t chw, dl_stream_t stream) {
  DL_CHECK_ARG(pred && xt && t && tables && x_prev && x0_est && batch > 0 && chw > 0 && T > 0, "dl_dpmpp_2m_step: bad args");
  DL_CHECK_ARG(mean_type == DL_MEAN_EPSILON || mean_type == DL_MEAN_XSTART || mean_type == DL_MEAN_V,
               "dl_dpmpp_2m_step: mean_type %d (a posterior-mean output has no place in an ODE solver)", mean_type);
  DL_CHECK_ARG(var_mode == DL_VAR_FIXED || var_mode == DL_VAR_LEARNED || var_mode == DL_VAR_LEARNED_RANGE,
               "dl_dpmpp_2m_step: var_mode %d", var_mode);
  DL_CHECK_ARG(a - a == 0.0f && b - b == 0.0f && c - c == 0.0f, "dl_dpmpp_2m_step: coefficients (%g, %g, %g) are not finite", (double)a,
               (double)b, (double)c);
  DL_CHECK_ARG(x0_last || c == 0.0f, "dl_dpmpp_2m_step: c != 0 needs x0_last");
  DL_CHECK_ARG(x0_est != x0_last && x_prev != x0_last && x_prev != x0_est, "dl_dpmpp_2m_step: an output aliases x0_last or the other");
  const int64_t n = batch * chw;
  if (c == 0.0f) x0_last = nullptr;  // (a first-order step reads no history)
  const bool gd = cfg_mul || x0_thr;
  const GaussTail<true> on{chw, cfg_mul, x0_thr};
  const GaussTail<false> off{chw};
#define DPMPP(H, G, HIST, TAIL)                                                                                                      \
  hipLaunchKernelGGL((dpmpp_2m_step_k<H, G, HIST>), ew_grid(n), 256, 0, (hipStream_t)stream, pred, pred_uncond, guidance, xt, x0_last, \
                     t, tables, T, mean_type, clamp_x, a, b, c, x_prev, x0_est, n, TAIL)
#define DPMPP_H(H)                                                              \
  do {                                                                          \
    if (x0_last) {                                                              \
      if (gd) DPMPP(H, true, true, on); else DPMPP(H, false, true, off);        \
    } else {                                                                    \
      if (gd) DPMPP(H, true, false, on); else DPMPP(H, false, false, off);      \
    }                                                                           \
  } while (0)
  if (var_mode == DL_VAR_FIXED) DPMPP_H(false); else DPMPP_H(true);
#undef DPMPP_H
#undef DPMPP
  DL_LAUNCH_CHECK();
  return DL_OK;
}

// CFG rescale (Lin et al., "Common Diffusion Noise Schedules and Sample Steps are Flawed", 2023, sec. 3.4): per sample
// r = 1 - phi + phi sqrt(S_c / S_o), S the centred sum of squares of the conditional prediction c and of the combined o = u + g (c - u).
// One workgroup per sample, two passes (mean first, then the deviations), double accumulators.  The reduction order is fixed: a
// thread's strided partial, a butterfly inside the wave, then the waves' partials summed in wave order; no floating-point atomics.
#define COEF_THREADS 1024
__device__ __forceinline__ double coef_block_sum(double v, double* part) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
  for (int w = 0; w < COEF_THREADS / 64; ++w) s += part[w];
  __syncthreads();  // `part` is free again
  return s;
}
__global__ __launch_bounds__(COEF_THREADS) void cfg_rescale_coef_k(const float* __restrict__ pred, const float* __restrict__ pu,
                                                                   float g, float phi, float* __restrict__ r, int64_t chw,
                                                                   int64_t stride) {
  __shared__ double part[COEF_THREADS / 64];
  const float* c = pred + (int64_t)blockIdx.x * stride;
  const float* u = pu + (int64_t)blockIdx.x * stride;
  double sc = 0.0, so = 0.0;
  for (int64_t i = threadIdx.x; i < chw; i += COEF_THREADS) {
    const float cv = c[i], uv = u[i];
    sc += (double)cv;
    so += (double)(uv + g * (cv - uv));
  }
  const double mc = coef_block_sum(sc, part) / (double)chw, mo = coef_block_sum(so, part) / (double)chw;
  double qc = 0.0, qo = 0.0;
  for (int64_t i = threadIdx.x; i < chw; i += COEF_THREADS) {
    const float cv = c[i], uv = u[i];
    const double dc = (double)cv - mc, dv = (double)(uv + g * (cv - uv)) - mo;
    qc += dc * dc;
    qo += dv * dv;
  }
  const double S_c = coef_block_sum(qc, part), S_o = coef_block_sum(qo, part);
  if (threadIdx.x == 0) r[blockIdx.x] = S_o > 0.0 ? (1.0f - phi) + phi * sqrtf((float)(S_c / S_o)) : 1.0f;
}
extern "C" int dl_cfg_rescale_coef(const float* pred, const float* pred_uncond, float guidance, float phi, float* r, int64_t batch,
                                   int64_t chw, int64_t sample_stride, dl_stream_t stream) {
  DL_CHECK_ARG(pred && pred_uncond && r && batch > 0 && chw > 0, "dl_cfg_rescale_coef: bad args");
  DL_CHECK_ARG(sample_stride == chw || sample_stride == 2 * chw, "dl_cfg_rescale_coef: sample_stride %lld is neither chw nor 2 chw",
               (long long)sample_stride);
  DL_CHECK_ARG(phi >= 0.0f && phi <= 1.0f, "dl_cfg_rescale_coef: phi %g outside [0, 1]", (double)phi);
  DL_CHECK_ARG(batch <= 0x7fffffff, "dl_cfg_rescale_coef: batch %lld", (long long)batch);
  hipLaunchKernelGGL(cfg_rescale_coef_k, (int)batch, COEF_THREADS, 0, (hipStream_t)stream, pred, pred_uncond, guidance, phi, r, chw,
                     sample_stride);
  DL_LAUNCH_CHECK();
  return DL_OK;
}

// Dynamic thresholding (Saharia et al., "Photorealistic Text-to-Image Diffusion Models with Deep Language Understanding", 2022): the
// p-quantile of |x0| of every sample, by torch.quantile's `linear` rule: a = lo + f (hi - lo), lo the k-th smallest key (0-based), hi
// the min(k + 1, n - 1)-th.  The selection is exact: the keys are non-negative floats, whose bit patterns order as uint32, and a radix
// select narrows the k-th smallest one 8-bit digit at a time, most significant first.  One workgroup per sample; per digit a 256-bin
// histogram in LDS (integer atomics, so the counts do not depend on the order of arrival), an inclusive scan of the bins, and the
// bin that holds rank k becomes the next digit of the answer.  After the last digit the rank inside the bin and the bin's count are
// those of the value lo itself, which gives the count of keys <= lo without another pass: with at least k + 2 of them hi = lo,
// otherwise one more pass takes the minimum of the keys > lo.  Keys of a sample of up to SEL_STAGE elements are computed once and
// staged in LDS (32 KiB); longer samples recompute them from global memory in every pass.
// Histogram contention: the leading digits of real data fall into two or three bins (the high exponent bits), so each wave first
// peels off the lanes that share the digit of its first active lane, twice, with one atomic per peel (__ballot over the 64 lanes),
// and only what is left issues an atomic per lane.
#define SEL_THREADS 1024
#define SEL_STAGE 8192
struct AbsKey {  // |x[i]|
  const float* x;
  __device__ __forceinline__ float operator()(int64_t i) const { return fabsf(x[i]); }
};
struct X0Key {  // |x0| as the GD step kernels form it: the same f32 expression on the same operands
  const float *pred, *pu, *xt;
  float g, mul;
  int has_mul, mean_type;
  float sab, ab, c1, c2;
  __device__ __forceinline__ float operator()(int64_t i) const {
    float o = pred[i];
    if (pu) {
      const float u = pu[i];
      o = u + g * (o - u);
    }
    if (has_mul) o *= mul;
    return fabsf(x_start_from(mean_type, o, xt[i], sab, ab, c1, c2));
  }
};
template <class Key>
__device__ __forceinline__ void select_abs(const Key& key, const int64_t n, const int64_t k, float& lo, float& hi) {
  __shared__ uint32_t s_keys[SEL_STAGE];
  __shared__ uint32_t s_hist[256];
  __shared__ uint32_t s_wave[4];
  __shared__ uint32_t s_pick[3];  // the chosen digit, the rank inside its bin, the bin's count
  __shared__ uint32_t s_min;
  const int tid = threadIdx.x, lane = tid & 63;
  const bool staged = n <= SEL_STAGE;
  uint32_t prefix = 0, mask = 0, rank = (uint32_t)k, count_eq = 0;
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    if (tid < 256) s_hist[tid] = 0;
    __syncthreads();
    for (int64_t base = 0; base < n; base += SEL_THREADS) {  // (every lane of a wave makes the same number of trips)
      const int64_t i = base + tid;
      uint32_t kb = 0;
      bool active = false;
      if (i < n) {
        if (pass == 0 || !staged) {
          kb = __float_as_uint(key(i));
          if (staged) s_keys[i] = kb;  // read back by this same thread only
        } else {
          kb = s_keys[i];
        }
        active = (kb & mask) == prefix;
      }
      const uint32_t digit = (kb >> shift) & 255u;
      for (int peel = 0; peel < 2; ++peel) {
        const unsigned long long m = __ballot(active);
        if (!m) break;
        const int leader = __ffsll((long long)m) - 1;
        const uint32_t d0 = __shfl(digit, leader);
        const bool same = active && digit == d0;
        const unsigned long long ms = __ballot(same);
        if (lane == leader) atomicAdd(&s_hist[d0], (uint32_t)__popcll(ms));
        if (same) active = false;
      }
      if (active) atomicAdd(&s_hist[digit], 1u);
    }
    __syncthreads();
    uint32_t c = 0, incl = 0;
    if (tid < 256) {  // waves 0..3: inclusive scan of the bins
      c = s_hist[tid];
      incl = c;
      for (int off = 1; off < 64; off <<= 1) {
        const uint32_t up = __shfl_up(incl, off);
        if (lane >= off) incl += up;
      }
      if (lane == 63) s_wave[tid >> 6] = incl;
    }
    __syncthreads();
    if (tid < 256) {
      for (int w = 0; w < (tid >> 6); ++w) incl += s_wave[w];
      const uint32_t excl = incl - c;
      if (rank >= excl && rank < incl) {  // exactly one bin: rank < the number of keys still in range
        s_pick[0] = (uint32_t)tid;
        s_pick[1] = rank - excl;
        s_pick[2] = c;
      }
    }
    __syncthreads();
    prefix |= s_pick[0] << shift;
    mask |= 255u << shift;
    rank = s_pick[1];
    count_eq = s_pick[2];
  }
  // prefix is the k-th smallest key; rank of its copies lie before position k, count_eq copies exist
  uint32_t hi_bits = prefix;
  if (k + 1 <= n - 1 && rank + 1 >= count_eq) {  // position k + 1 exists and holds a larger key: the smallest one > lo
    if (tid == 0) s_min = 0xffffffffu;
    __syncthreads();
    uint32_t best = 0xffffffffu;
    for (int64_t i = tid; i < n; i += SEL_THREADS) {
      const uint32_t kb = staged ? s_keys[i] : __float_as_uint(key(i));
      if (kb > prefix && kb < best) best = kb;
    }
    for (int off = 32; off > 0; off >>= 1) {
      const uint32_t other = __shfl_xor(best, off);
      best = other < best ? other : best;
    }
    if (lane == 0) atomicMin(&s_min, best);
    __syncthreads();
    hi_bits = s_min;
  }
  lo = __uint_as_float(prefix);
  hi = __uint_as_float(hi_bits);
}
__global__ __launch_bounds__(SEL_THREADS) void abs_quantile_rows_k(const float* __restrict__ x, int64_t n, int64_t k, float f,
                                                                   float* __restrict__ q, float* __restrict__ lohi) {
  const int64_t b = blockIdx.x;
  const AbsKey key{x + b * n};
  float lo, hi;
  select_abs(key, n, k, lo, hi);
  if (threadIdx.x == 0) {
    q[b] = lo + f * (hi - lo);
    if (lohi) {
      lohi[2 * b] = lo;
      lohi[2 * b + 1] = hi;
    }
  }
}
__global__ __launch_bounds__(SEL_THREADS) void x0_threshold_k(const float* __restrict__ pred, const float* __restrict__ pu, float g,
                                                              const float* __restrict__ mul, const float* __restrict__ xt,
                                                              const int32_t* __restrict__ t, const float* __restrict__ tab, int32_t T,
                                                              int mean_type, const float* __restrict__ coefs, int64_t k, float f,
                                                              float cap, float* __restrict__ s, float* __restrict__ lohi,
                                                              int64_t chw, int64_t stride) {
  const int64_t b = blockIdx.x;
  const int32_t ti = t[b];
  const X0Key key{pred + b * stride, pu ? pu + b * stride : nullptr, xt + b * chw, g, mul ? mul[b] : 1.0f, mul != nullptr, mean_type,
                  tab[ti], tab[T + ti], coefs ? coefs[ti] : 1.0f, coefs ? coefs[T + ti] : 0.0f};
  float lo, hi;
  select_abs(key, chw, k, lo, hi);
  if (threadIdx.x == 0) {
    const float q = lo + f * (hi - lo);
    s[b] = fminf(fmaxf(q, 1.0f), cap);
    if (lohi) {
      lohi[2 * b] = lo;
      lohi[2 * b + 1] = hi;
    }
  }
}
static int quantile_check(const char* who, int64_t batch, int64_t n, int64_t k, float f) {
  DL_CHECK_ARG(batch > 0 && batch <= 0x7fffffff && n > 0 && n <= 0x7fffffff, "%s: batch %lld, n %lld", who, (long long)batch,
               (long long)n);
  DL_CHECK_ARG(k >= 0 && k < n, "%s: k %lld outside [0, n = %lld)", who, (long long)k, (long long)n);
  DL_CHECK_ARG(f >= 0.0f && f < 1.0f, "%s: f %g outside [0, 1)", who, (double)f);
  return DL_OK;
}
extern "C" int dl_abs_quantile_rows(const float* x, int64_t k, float f, float* q, float* lohi, int64_t batch, int64_t n,
                                    dl_stream_t stream) {
  DL_CHECK_ARG(x && q, "dl_abs_quantile_rows: bad args");
  if (int rc = quantile_check("dl_abs_quantile_rows", batch, n, k, f)) return rc;
  hipLaunchKernelGGL(abs_quantile_rows_k, (int)batch, SEL_THREADS, 0, (hipStream_t)stream, x, n, k, f, q, lohi);
  DL_LAUNCH_CHECK();
  return DL_OK;
}
extern "C" int dl_x0_threshold(const float* pred, const float* pred_uncond, float guidance, const float* cfg_mul, const float* xt,
                               const int32_t* t, const float* tables, int32_t T, int mean_type, const float* coefs, int64_t k, float f,
                               float threshold_max, float* s, float* lohi, int64_t batch, int64_t chw, int64_t sample_stride,
                               dl_stream_t stream) {
  DL_CHECK_ARG(pred && xt && t && tables && s && T > 0, "dl_x0_threshold: bad args");
  if (int rc = quantile_check("dl_x0_threshold", batch, chw, k, f)) return rc;
  DL_CHECK_ARG(sample_stride == chw || sample_stride == 2 * chw, "dl_x0_threshold: sample_stride %lld is neither chw nor 2 chw",
               (long long)sample_stride);
  DL_CHECK_ARG(mean_type >= DL_MEAN_EPSILON && mean_type <= DL_MEAN_V, "dl_x0_threshold: mean_type %d", mean_type);
  DL_CHECK_ARG(mean_type != DL_MEAN_XPREV || coefs, "dl_x0_threshold: xprev needs coefs");
  DL_CHECK_ARG(threshold_max >= 1.0f, "dl_x0_threshold: threshold_max %g < 1 (INFINITY = no cap)", (double)threshold_max);
  hipLaunchKernelGGL(x0_threshold_k, (int)batch, SEL_THREADS, 0, (hipStream_t)stream, pred, pred_uncond, guidance, cfg_mul, xt, t,
                     tables, T, mean_type, coefs, k, f, threshold_max, s, lohi, chw, sample_stride);
  DL_LAUNCH_CHECK();
  return DL_OK;
}

// ---------------------------------------------------------------- image-to-image / inpainting (Flow.denoise, GaussianDiffusion.denoise)
// The known region of SDEdit (Meng et al. 2022) / RePaint (Lugmayr et al. 2022) sampling, after a sampler step: known = a ref + b noise
// is the reference image at the noise level the step arrived at, and out = x where the mask generates, known where it keeps, the
// convex mix on a soft edge.  m >= 1 and m <= 0 are selects, so nothing non-finite crosses from the discarded side and the kept side
// is returned bit for bit.  Without a mask (MASK false) out = known: RePaint's re-noise x_t = a x_prev + b noise between the repeats of
// a step.  x, ref and out carry no __restrict__: out may be x or ref (every element is read before it alone is written).
template <bool MASK>
__global__ void inpaint_blend_k(const float* x, const float* ref, const float* __restrict__ noise, const float* __restrict__ mask,
                                float a, float b, float* out, int64_t n, int64_t chw, int64_t hw, int mask_full) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    float known = a * ref[i];
    if (noise) known += b * noise[i];
    if (MASK) {
      const float m = mask[mask_full ? i : (i / chw) * hw + i % hw];
      const float xi = x[i];
      out[i] = m >= 1.0f ? xi : (m <= 0.0f ? known : m * xi + (1.0f - m) * known);
    } else {
      out[i] = known;
    }
  }
}
extern "C" int dl_inpaint_blend(const float* x, const float* ref, const float* noise, const float* mask, float a, float b,
                                float* out, int64_t batch, int64_t channels, int64_t hw, int64_t mask_channels,
                                dl_stream_t stream) {
  DL_CHECK_ARG(ref && out, "dl_inpaint_blend: bad args (ref, out non-null)");
  DL_CHECK_ARG(batch > 0 && channels > 0 && hw > 0, "dl_inpaint_blend: bad args (batch, channels, hw > 0)");
  DL_CHECK_ARG(noise || b == 0.0f, "dl_inpaint_blend: b != 0 needs noise");
  DL_CHECK_ARG((mask != nullptr) == (x != nullptr), "dl_inpaint_blend: a mask needs x, and x needs a mask (mask NULL: out = a ref + b noise)");
  DL_CHECK_ARG(!mask || mask_channels == 1 || mask_channels == channels, "dl_inpaint_blend: mask_channels %lld is neither 1 nor channels %lld",
               (long long)mask_channels, (long long)channels);
  const int64_t chw = channels * hw, n = batch * chw;
  if (b == 0.0f) noise = nullptr;  // (the final Gaussian step: known = ref, nothing is read from noise)
  if (mask)
    hipLaunchKernelGGL(inpaint_blend_k<true>, ew_grid(n), 256, 0, (hipStream_t)stream, x, ref, noise, mask, a, b, out, n, chw, hw,
                       (int)(mask_channels == channels));
  else
    hipLaunchKernelGGL(inpaint_blend_k<false>, ew_grid(n), 256, 0, (hipStream_t)stream, x, ref, noise, mask, a, b, out, n, chw, hw, 0);
  DL_LAUNCH_CHECK();
  return DL_OK;
}
