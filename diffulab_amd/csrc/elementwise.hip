// HBM-bound kernels: diffusion heads (noising, losses), sampler steps, optimizer, casts.
// All are float4 / 16-byte vectorised grid-stride loops (cdna_hip_programming.md Appendix B "Element-wise").
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include "common.h"

// ---------------------------------------------------------------- error plumbing / library info
static thread_local char g_err[512] = "";
void dl_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
extern "C" const char* dl_last_error(void) { return g_err; }
static thread_local int g_wg_cap = 0;
void dl_set_wg_cap(int cap) { g_wg_cap = cap > 0 ? cap : 0; }
int dl_get_wg_cap() { return g_wg_cap; }
int dl_wg_budget(int n_cu) {
  int n = (g_wg_cap > 0 && g_wg_cap < n_cu) ? g_wg_cap : n_cu;
  return n < 8 ? 8 : n;
}
extern "C" int dl_version(void) { return 100; }
extern "C" int dl_device_info(int device, int* cu, int* lds, int64_t* hbm, char* arch, int arch_len) {
  hipDeviceProp_t p;
  hipError_t e = hipGetDeviceProperties(&p, device);
  if (e != hipSuccess) {
    dl_set_error("hipGetDeviceProperties: %s", hipGetErrorString(e));
    return DL_ERR_LAUNCH;
  }
  if (cu) *cu = p.multiProcessorCount;
  if (lds) *lds = (int)p.maxSharedMemoryPerMultiProcessor;
  if (hbm) *hbm = (int64_t)p.totalGlobalMem;
  if (arch && arch_len > 0) {
    strncpy(arch, p.gcnArchName, arch_len - 1);
    arch[arch_len - 1] = 0;
  }
  return DL_OK;
}

// HIP stream restricted to a subset of the compute units (hipExtStreamCreateWithCUMask): the engines put the weight-gradient
// GEMMs on such a stream so that they cannot crowd the latency-bound kernels of the main dependency chain off the CUs.
extern "C" int dl_stream_create_masked(const uint32_t* cu_mask, int words, void** stream_out) {
  DL_CHECK_ARG(cu_mask && words > 0 && stream_out, "dl_stream_create_masked: bad args");
  hipStream_t st = nullptr;
  const hipError_t e = hipExtStreamCreateWithCUMask(&st, (uint32_t)words, cu_mask);
  if (e != hipSuccess) {
    dl_set_error("hipExtStreamCreateWithCUMask: %s", hipGetErrorString(e));
    return DL_ERR_LAUNCH;
  }
  *stream_out = (void*)st;
  return DL_OK;
}
// HIP stream of the LOWEST priority the device offers (the side stream of the weight gradients: when both queues have workgroups
// ready the dispatcher serves the main chain's first); *range_out = {least, greatest} as hipDeviceGetStreamPriorityRange reports it
extern "C" int dl_stream_create_low_priority(void** stream_out, int* range_out) {
  DL_CHECK_ARG(stream_out, "dl_stream_create_low_priority: bad args");
  int least = 0, greatest = 0;
  hipError_t e = hipDeviceGetStreamPriorityRange(&least, &greatest);
  if (e != hipSuccess) {
    dl_set_error("hipDeviceGetStreamPriorityRange: %s", hipGetErrorString(e));
    return DL_ERR_LAUNCH;
  }
  if (range_out) {
    range_out[0] = least;
    range_out[1] = greatest;
  }
  hipStream_t st = nullptr;
  e = hipStreamCreateWithPriority(&st, hipStreamNonBlocking, least);
  if (e != hipSuccess) {
    dl_set_error("hipStreamCreateWithPriority: %s", hipGetErrorString(e));
    return DL_ERR_LAUNCH;
  }
  *stream_out = (void*)st;
  return DL_OK;
}
extern "C" int dl_stream_destroy(void* stream) {
  if (stream && hipStreamDestroy((hipStream_t)stream) != hipSuccess) return DL_ERR_LAUNCH;
  return DL_OK;
}

static inline int ew_grid(int64_t nvec, int threads = 256) {
  int64_t g = (nvec + threads - 1) / threads;
  if (g > 2048) g = 2048;  // 256 CUs x 8 blocks, grid-stride beyond that
  if (g < 1) g = 1;
  return (int)g;
}

// ---------------------------------------------------------------- noising
// z = (1-t) x + t eps; chw % 4 == 0 fast path works on float4, else scalar
template <bool VEC>
__global__ void flow_add_noise_k(const float* __restrict__ x, const float* __restrict__ e,
                                 const float* __restrict__ t, float* __restrict__ z, int64_t n, int64_t chw) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  if (VEC) {
    const int64_t nv = n >> 2, cv = chw >> 2;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += stride) {
      const float tt = t[i / cv], at = 1.0f - tt;
      const float4 a = ((const float4*)x)[i], b = ((const float4*)e)[i];
      float4 o;
      o.x = at * a.x + tt * b.x;
      o.y = at * a.y + tt * b.y;
      o.z = at * a.z + tt * b.z;
      o.w = at * a.w + tt * b.w;
      ((float4*)z)[i] = o;
    }
  } else {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
      const float tt = t[i / chw];
      z[i] = (1.0f - tt) * x[i] + tt * e[i];
    }
  }
}
extern "C" int dl_flow_add_noise(const float* x, const float* noise, const float* t, float* z, int64_t batch,
                                 int64_t chw, dl_stream_t stream) {
  DL_CHECK_ARG(x && noise && t && z && batch > 0 && chw > 0, "dl_flow_add_noise: bad args");
  const int64_t n = batch * chw;
  if (chw % 4 == 0)
    hipLaunchKernelGGL(flow_add_noise_k<true>, ew_grid(n / 4), 256, 0, (hipStream_t)stream, x, noise, t, z, n, chw);
  else
    hipLaunchKernelGGL(flow_add_noise_k<false>, ew_grid(n), 256, 0, (hipStream_t)stream, x, noise, t, z, n, chw);
  DL_LAUNCH_CHECK();
  return DL_OK;
}

__global__ void ddpm_add_noise_k(const float* __restrict__ x, const float* __restrict__ e,
                                 const int32_t* __restrict__ t, const float* __restrict__ sqrt_ab,
                                 const float* __restrict__ ab, float* __restrict__ o, int64_t n, int64_t chw) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const int32_t ti = t[i / chw];
    const float ca = sqrt_ab[ti];
    const float cb = sqrtf(1.0f - ab[ti]);  // gd.py:340: sqrt evaluated in fp32 after the .float() gather
    o[i] = ca * x[i] + cb * e[i];
  }
}
extern "C" int dl_ddpm_add_noise(const float* x, const float* noise, const int32_t* t, const float* sqrt_ab,
                                 const float* ab, float* xt, int64_t batch, int64_t chw, dl_stream_t stream) {
  DL_CHECK_ARG(x && noise && t && sqrt_ab && ab && xt && batch > 0 && chw > 0, "dl_ddpm_add_noise: bad args");
  const int64_t n = batch * chw;
  hipLaunchKernelGGL(ddpm_add_noise_k, ew_grid(n), 256, 0, (hipStream_t)stream, x, noise, t, sqrt_ab, ab, xt, n, chw);
  DL_LAUNCH_CHECK();
  return DL_OK;
}

// ---------------------------------------------------------------- MSE heads
#define MSE_BLOCK 256
#define MSE_ELEMS_PER_BLOCK (MSE_BLOCK * 16)
extern "C" int64_t dl_mse_loss_partials(int64_t n) { return (n + MSE_ELEMS_PER_BLOCK - 1) / MSE_ELEMS_PER_BLOCK; }

__global__ void mse_partial_k(const float* __restrict__ pred, const float* __restrict__ a,
                              const float* __restrict__ b, float* __restrict__ partial, int64_t n, int mode) {
  __shared__ float red[MSE_BLOCK / DL_WAVE];
  const int64_t base = (int64_t)blockIdx.x * MSE_ELEMS_PER_BLOCK;
  float acc = 0.f;
#pragma unroll 4
  for (int j = 0; j < 16; ++j) {
    const int64_t i = base + (int64_t)j * MSE_BLOCK + threadIdx.x;
    if (i < n) {
      const float tgt = (mode == DL_LOSS_FLOW) ? (a[i] - b[i]) : a[i];
      const float d = tgt - pred[i];
      acc += d * d;
    }
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = 0.f;
    for (int w = 0; w < MSE_BLOCK / DL_WAVE; ++w) s += red[w];
    partial[blockIdx.x] = s;
  }
}
__global__ void mse_final_k(const float* __restrict__ partial, float* __restrict__ loss, int64_t np, float inv_n) {
  __shared__ float red[256 / DL_WAVE];
  float acc = 0.f;
  for (int64_t i = threadIdx.x; i < np; i += 256) acc += partial[i];
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) *loss = (red[0] + red[1] + red[2] + red[3]) * inv_n;
}
extern "C" int dl_mse_loss_fwd(const float* pred, const float* a, const float* b, float* partial, float* loss,
                               int64_t n, int mode, dl_stream_t stream) {
  DL_CHECK_ARG(pred && a && partial && loss && n > 0, "dl_mse_loss_fwd: bad args");
  DL_CHECK_ARG(mode == DL_LOSS_EPS || b, "dl_mse_loss_fwd: flow mode needs b (x0)");
  const int64_t np = dl_mse_loss_partials(n);
  hipLaunchKernelGGL(mse_partial_k, (int)np, MSE_BLOCK, 0, (hipStream_t)stream, pred, a, b, partial, n, mode);
  hipLaunchKernelGGL(mse_final_k, 1, 256, 0, (hipStream_t)stream, partial, loss, np, (float)(1.0 / (double)n));
  DL_LAUNCH_CHECK();
  return DL_OK;
}
__global__ void mse_bwd_k(const float* __restrict__ pred, const float* __restrict__ a, const float* __restrict__ b,
                          float coef, const float* __restrict__ gdev, float* __restrict__ dpred, int64_t n, int mode) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  if (gdev) coef *= *gdev;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const float tgt = (mode == DL_LOSS_FLOW) ? (a[i] - b[i]) : a[i];
    dpred[i] = coef * (pred[i] - tgt);
  }
}
extern "C" int dl_mse_loss_bwd(const float* pred, const float* a, const float* b, float gscale,
                               const float* gscale_dev, float* dpred, int64_t n, int mode, dl_stream_t stream) {
  DL_CHECK_ARG(pred && a && dpred && n > 0, "dl_mse_loss_bwd: bad args");
  DL_CHECK_ARG(mode == DL_LOSS_EPS || b, "dl_mse_loss_bwd: flow mode needs b (x0)");
  const float coef = (float)(2.0 * (double)gscale / (double)n);
  hipLaunchKernelGGL(mse_bwd_k, ew_grid(n), 256, 0, (hipStream_t)stream, pred, a, b, coef, gscale_dev, dpred, n, mode);
  DL_LAUNCH_CHECK();
  return DL_OK;
}

__global__ void x_to_v_k(const float* __restrict__ z, const float* __restrict__ xh, const float* __restrict__ t,
                         float* __restrict__ v, int64_t n, int64_t chw) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    v[i] = (z[i] - xh[i]) / t[i / chw];
}
__global__ void x_to_v_bwd_k(const float* __restrict__ dv, const float* __restrict__ t, float* __restrict__ dx,
                             int64_t n, int64_t chw) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    dx[i] = -dv[i] / t[i / chw];
}
extern "C" int dl_flow_x_to_v(const float* z, const float* xhat, const float* t, float* v, int64_t batch,
                              int64_t chw, dl_stream_t stream) {
  DL_CHECK_ARG(z && xhat && t && v && batch > 0 && chw > 0, "dl_flow_x_to_v: bad args");
  hipLaunchKernelGGL(x_to_v_k, ew_grid(batch * chw), 256, 0, (hipStream_t)stream, z, xhat, t, v, batch * chw, chw);
  DL_LAUNCH_CHECK();
  return DL_OK;
}
extern "C" int dl_flow_x_to_v_bwd(const float* dv, const float* t, float* dxhat, int64_t batch, int64_t chw,
                                  dl_stream_t stream) {
  DL_CHECK_ARG(dv && t && dxhat && batch > 0 && chw > 0, "dl_flow_x_to_v_bwd: bad args");
  hipLaunchKernelGGL(x_to_v_bwd_k, ew_grid(batch * chw), 256, 0, (hipStream_t)stream, dv, t, dxhat, batch * chw, chw);
  DL_LAUNCH_CHECK();
  return DL_OK;
}

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
extern "C" int dl_euler_step(const float* x, const float* v, const float* v_uncond, float guidance, float t_curr,
                             float dt, float* x_prev, float* x0_est, int64_t n, dl_stream_t stream) {
  DL_CHECK_ARG(x && v && x_prev && n > 0, "dl_euler_step: bad args");
  hipLaunchKernelGGL(euler_step_k<false>, ew_grid(n), 256, 0, (hipStream_t)stream, x, v, v_uncond, guidance, t_curr, dt,
                     x_prev, x0_est, FlowTail<false>{n});
  DL_LAUNCH_CHECK();
  return DL_OK;
}
extern "C" int dl_euler_step_g(const float* x, const float* v, const float* v_uncond, float guidance, const float* cfg_mul,
                               float t_curr, float dt, float* x_prev, float* x0_est, int64_t batch, int64_t chw,
                               dl_stream_t stream) {
  DL_CHECK_ARG(x && v && x_prev && batch > 0 && chw > 0, "dl_euler_step_g: bad args");
  const int64_t n = batch * chw;
  if (!cfg_mul) return dl_euler_step(x, v, v_uncond, guidance, t_curr, dt, x_prev, x0_est, n, stream);
  hipLaunchKernelGGL(euler_step_k<true>, ew_grid(n), 256, 0, (hipStream_t)stream, x, v, v_uncond, guidance, t_curr, dt,
                     x_prev, x0_est, FlowTail<true>{n, cfg_mul, chw});
  DL_LAUNCH_CHECK();
  return DL_OK;
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
extern "C" int dl_euler_maruyama_step(const float* x, const float* v, const float* v_uncond, float guidance,
                                      const float* noise, const float* x_prev_in, float t_curr, float dt,
                                      float sigma, float std, float* x_prev, float* mean, float* x0_est,
                                      float* logprob, int64_t n, dl_stream_t stream) {
  DL_CHECK_ARG(x && v && x_prev && n > 0, "dl_euler_maruyama_step: bad args");
  DL_CHECK_ARG((noise != nullptr) != (x_prev_in != nullptr), "dl_euler_maruyama_step: exactly one of noise/x_prev_in");
  const float drift_c = (float)((double)sigma * (double)sigma / (2.0 * (double)t_curr));
  hipLaunchKernelGGL(em_step_k<false>, ew_grid(n), 256, 0, (hipStream_t)stream, x, v, v_uncond, guidance, noise, x_prev_in,
                     t_curr, dt, drift_c, std, logf(std), x_prev, mean, x0_est, logprob, FlowTail<false>{n});
  DL_LAUNCH_CHECK();
  return DL_OK;
}
extern "C" int dl_euler_maruyama_step_g(const float* x, const float* v, const float* v_uncond, float guidance,
                                        const float* cfg_mul, const float* noise, const float* x_prev_in, float t_curr, float dt,
                                        float sigma, float std, float* x_prev, float* mean, float* x0_est, float* logprob,
                                        int64_t batch, int64_t chw, dl_stream_t stream) {
  DL_CHECK_ARG(x && v && x_prev && batch > 0 && chw > 0, "dl_euler_maruyama_step_g: bad args");
  DL_CHECK_ARG((noise != nullptr) != (x_prev_in != nullptr), "dl_euler_maruyama_step_g: exactly one of noise/x_prev_in");
  const int64_t n = batch * chw;
  if (!cfg_mul)
    return dl_euler_maruyama_step(x, v, v_uncond, guidance, noise, x_prev_in, t_curr, dt, sigma, std, x_prev, mean, x0_est, logprob,
                                  n, stream);
  const float drift_c = (float)((double)sigma * (double)sigma / (2.0 * (double)t_curr));
  hipLaunchKernelGGL(em_step_k<true>, ew_grid(n), 256, 0, (hipStream_t)stream, x, v, v_uncond, guidance, noise, x_prev_in,
                     t_curr, dt, drift_c, std, logf(std), x_prev, mean, x0_est, logprob, FlowTail<true>{n, cfg_mul, chw});
  DL_LAUNCH_CHECK();
  return DL_OK;
}

__device__ __forceinline__ float x_start_from(int mean_type, float out, float xt, float sab, float ab, float c1,
                                              float c2) {
  if (mean_type == DL_MEAN_XSTART) return out;
  if (mean_type == DL_MEAN_EPSILON) return (1.0f / sab) * xt - (sqrtf(1.0f - ab) / sab) * out;  // ddpm.py:118-121
  if (mean_type == DL_MEAN_V) return sab * xt - sqrtf(1.0f - ab) * out;  // Salimans & Ho (2022): v = sab eps - sqrt(1 - ab) x0
  return (1.0f / c1) * out - (c2 / c1) * xt;                                                    // ddpm.py:99-102
}
// dynamic thresholding (Saharia et al., Imagen, 2022): x0 clamped to the sample's own threshold s >= 1 and divided by it
__device__ __forceinline__ float threshold_x0(float x0, float s) { return fminf(fmaxf(x0, -s), s) / s; }

template <bool GD>
__global__ void ddpm_step_k(const float* __restrict__ pred, const float* __restrict__ pu, float g,
                            const float* __restrict__ xt, const float* __restrict__ noise,
                            const int32_t* __restrict__ t, const float* __restrict__ tab, int32_t T, int mean_type,
                            int clamp_x, float* __restrict__ xp, float* __restrict__ x0o, float* __restrict__ mo,
                            float* __restrict__ so, float* __restrict__ lp, int64_t n, const GaussTail<GD> tail) {
  const int64_t chw = tail.chw;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const int64_t b = i / chw;
    const int32_t ti = t[b];
    const float sab = tab[ti], ab = tab[T + ti], c1 = tab[2 * T + ti], c2 = tab[3 * T + ti];
    const float var = tab[4 * T + ti], lv = tab[5 * T + ti];
    float o = pred[i];
    if (pu) {
      const float u = pu[i];
      o = u + g * (o - u);
    }
    if constexpr (GD) {
      if (tail.mul) o *= tail.mul[b];
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
extern "C" int dl_ddpm_step(const float* pred, const float* pred_uncond, float guidance, const float* xt,
                            const float* noise, const int32_t* t, const float* tables, int32_t T, int mean_type,
                            int clamp_x, float* x_prev, float* x0_est, float* mean, float* std, float* logprob,
                            int64_t batch, int64_t chw, dl_stream_t stream) {
  DL_CHECK_ARG(pred && xt && noise && t && tables && x_prev && batch > 0 && chw > 0 && T > 0, "dl_ddpm_step: bad args");
  DL_CHECK_ARG(mean_type >= 0 && mean_type <= 2, "dl_ddpm_step: mean_type %d", mean_type);
  const int64_t n = batch * chw;
  hipLaunchKernelGGL(ddpm_step_k<false>, ew_grid(n), 256, 0, (hipStream_t)stream, pred, pred_uncond, guidance, xt, noise, t,
                     tables, T, mean_type, clamp_x, x_prev, x0_est, mean, std, logprob, n, GaussTail<false>{chw});
  DL_LAUNCH_CHECK();
  return DL_OK;
}

// learned variances (ddpm.py:212-222, 268-282): pred / pu are [B, 2 chw], element (b, r) has its mean output at b 2chw + r and its raw
// variance output at b 2chw + chw + r, both read in place.  tab: f32 [6][T] = sqrt_ab, ab, coef1, coef2, posterior_log_variance_clipped,
// betas.  The log-variance of one element, shared with the hybrid loss below:
__device__ __forceinline__ float learned_log_var(int var_mode, float v, float min_log, float beta) {
  if (var_mode == DL_VAR_LEARNED) return v;
  const float w = (v + 1.0f) / 2.0f;  // ddpm.py:218-221; log(betas[t]) in f32 after the gather
  return w * logf(beta) + (1.0f - w) * min_log;
}
template <bool GD>
__global__ void ddpm_step_lv_k(const float* __restrict__ pred, const float* __restrict__ pu, float g,
                               const float* __restrict__ xt, const float* __restrict__ noise,
                               const int32_t* __restrict__ t, const float* __restrict__ tab, int32_t T, int mean_type,
                               int var_mode, int clamp_x, float* __restrict__ xp, float* __restrict__ x0o,
                               float* __restrict__ mo, float* __restrict__ so, float* __restrict__ lp, int64_t n,
                               const GaussTail<GD> tail) {
  const int64_t chw = tail.chw;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const int64_t b = i / chw;
    const int32_t ti = t[b];
    const float sab = tab[ti], ab = tab[T + ti], c1 = tab[2 * T + ti], c2 = tab[3 * T + ti];
    const float min_log = tab[4 * T + ti], beta = tab[5 * T + ti];
    const int64_t pi = i + b * chw;
    float o = pred[pi], v = pred[pi + chw];
    if (pu) {  // the CFG combine acts on the whole 2C tensor before the chunk (gaussian_diffusion.py:253-255)
      const float uo = pu[pi], uv = pu[pi + chw];
      o = uo + g * (o - uo);
      v = uv + g * (v - uv);
    }
    if constexpr (GD) {  // the mean half only: the variance half keeps the plain combine
      if (tail.mul) o *= tail.mul[b];
    }
    const float lv = learned_log_var(var_mode, v, min_log, beta);
    const float var = expf(lv);
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
extern "C" int dl_ddpm_step_lv(const float* pred, const float* pred_uncond, float guidance, const float* xt,
                               const float* noise, const int32_t* t, const float* tables, int32_t T, int mean_type,
                               int var_mode, int clamp_x, float* x_prev, float* x0_est, float* mean, float* std,
                               float* logprob, int64_t batch, int64_t chw, dl_stream_t stream) {
  DL_CHECK_ARG(pred && xt && noise && t && tables && x_prev && batch > 0 && chw > 0 && T > 0, "dl_ddpm_step_lv: bad args");
  DL_CHECK_ARG(mean_type >= 0 && mean_type <= 2, "dl_ddpm_step_lv: mean_type %d", mean_type);
  DL_CHECK_ARG(var_mode == DL_VAR_LEARNED || var_mode == DL_VAR_LEARNED_RANGE, "dl_ddpm_step_lv: var_mode %d", var_mode);
  const int64_t n = batch * chw;
  hipLaunchKernelGGL(ddpm_step_lv_k<false>, ew_grid(n), 256, 0, (hipStream_t)stream, pred, pred_uncond, guidance, xt, noise, t,
                     tables, T, mean_type, var_mode, clamp_x, x_prev, x0_est, mean, std, logprob, n, GaussTail<false>{chw});
  DL_LAUNCH_CHECK();
  return DL_OK;
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
extern "C" int dl_ddim_step(const float* pred, const float* pred_uncond, float guidance, const float* xt,
                            const float* noise, const int32_t* t, const float* tables, int32_t T, int mean_type,
                            const float* ddpm_coefs, int clamp_x, float eta, float* x_prev, float* x0_est,
                            float* mean, float* std, float* logprob, int64_t batch, int64_t chw,
                            dl_stream_t stream) {
  DL_CHECK_ARG(pred && xt && noise && t && tables && x_prev && batch > 0 && chw > 0 && T > 0, "dl_ddim_step: bad args");
  DL_CHECK_ARG(mean_type >= 0 && mean_type <= 2, "dl_ddim_step: mean_type %d", mean_type);
  DL_CHECK_ARG(mean_type != DL_MEAN_XPREV || ddpm_coefs, "dl_ddim_step: xprev needs ddpm_coefs");
  const int64_t n = batch * chw;
  hipLaunchKernelGGL((ddim_step_k<false, false>), ew_grid(n), 256, 0, (hipStream_t)stream, pred, pred_uncond, guidance, xt, noise, t,
                     tables, T, mean_type, ddpm_coefs, clamp_x, eta, x_prev, x0_est, mean, std, logprob, n, GaussTail<false>{chw});
  DL_LAUNCH_CHECK();
  return DL_OK;
}
extern "C" int dl_ddim_step_lv(const float* pred, const float* pred_uncond, float guidance, const float* xt,
                               const float* noise, const int32_t* t, const float* tables, int32_t T, int mean_type,
                               const float* ddpm_coefs, int clamp_x, float eta, float* x_prev, float* x0_est,
                               float* mean, float* std, float* logprob, int64_t batch, int64_t chw,
                               dl_stream_t stream) {
  DL_CHECK_ARG(pred && xt && noise && t && tables && x_prev && batch > 0 && chw > 0 && T > 0, "dl_ddim_step_lv: bad args");
  DL_CHECK_ARG(mean_type >= 0 && mean_type <= 2, "dl_ddim_step_lv: mean_type %d", mean_type);
  DL_CHECK_ARG(mean_type != DL_MEAN_XPREV || ddpm_coefs, "dl_ddim_step_lv: xprev needs ddpm_coefs");
  const int64_t n = batch * chw;
  hipLaunchKernelGGL((ddim_step_k<true, false>), ew_grid(n), 256, 0, (hipStream_t)stream, pred, pred_uncond, guidance, xt, noise, t,
                     tables, T, mean_type, ddpm_coefs, clamp_x, eta, x_prev, x0_est, mean, std, logprob, n, GaussTail<false>{chw});
  DL_LAUNCH_CHECK();
  return DL_OK;
}

// v-prediction (Salimans & Ho 2022) through the same kernel bodies: x_start_from's DL_MEAN_V case.  One entry point per sampler takes
// the [B, chw] prediction of a fixed-variance model (DL_VAR_FIXED: tables as for dl_ddpm_step / dl_ddim_step) and the [B, 2 chw] one
// of a learned-variance model (tables as for the _lv entry points).
static int step_v_check(const char* who, const void* pred, const void* xt, const void* noise, const void* t, const void* tables,
                        const void* x_prev, int32_t T, int var_mode, int64_t batch, int64_t chw) {
  DL_CHECK_ARG(pred && xt && noise && t && tables && x_prev && batch > 0 && chw > 0 && T > 0, "%s: bad args", who);
  DL_CHECK_ARG(var_mode == DL_VAR_FIXED || var_mode == DL_VAR_LEARNED || var_mode == DL_VAR_LEARNED_RANGE, "%s: var_mode %d", who,
               var_mode);
  return DL_OK;
}
extern "C" int dl_ddpm_step_v(const float* pred, const float* pred_uncond, float guidance, const float* xt, const float* noise,
                              const int32_t* t, const float* tables, int32_t T, int var_mode, int clamp_x, float* x_prev,
                              float* x0_est, float* mean, float* std, float* logprob, int64_t batch, int64_t chw,
                              dl_stream_t stream) {
  if (int rc = step_v_check("dl_ddpm_step_v", pred, xt, noise, t, tables, x_prev, T, var_mode, batch, chw)) return rc;
  const int64_t n = batch * chw;
  if (var_mode == DL_VAR_FIXED)
    hipLaunchKernelGGL(ddpm_step_k<false>, ew_grid(n), 256, 0, (hipStream_t)stream, pred, pred_uncond, guidance, xt, noise, t, tables, T,
                       DL_MEAN_V, clamp_x, x_prev, x0_est, mean, std, logprob, n, GaussTail<false>{chw});
  else
    hipLaunchKernelGGL(ddpm_step_lv_k<false>, ew_grid(n), 256, 0, (hipStream_t)stream, pred, pred_uncond, guidance, xt, noise, t, tables,
                       T, DL_MEAN_V, var_mode, clamp_x, x_prev, x0_est, mean, std, logprob, n, GaussTail<false>{chw});
  DL_LAUNCH_CHECK();
  return DL_OK;
}
extern "C" int dl_ddim_step_v(const float* pred, const float* pred_uncond, float guidance, const float* xt, const float* noise,
                              const int32_t* t, const float* tables, int32_t T, int var_mode, int clamp_x, float eta,
                              float* x_prev, float* x0_est, float* mean, float* std, float* logprob, int64_t batch, int64_t chw,
                              dl_stream_t stream) {
  if (int rc = step_v_check("dl_ddim_step_v", pred, xt, noise, t, tables, x_prev, T, var_mode, batch, chw)) return rc;
  const int64_t n = batch * chw;
  const float* no_coefs = nullptr;  // the posterior-mean coefficients serve DL_MEAN_XPREV only
  if (var_mode == DL_VAR_FIXED)
    hipLaunchKernelGGL((ddim_step_k<false, false>), ew_grid(n), 256, 0, (hipStream_t)stream, pred, pred_uncond, guidance, xt, noise, t,
                       tables, T, DL_MEAN_V, no_coefs, clamp_x, eta, x_prev, x0_est, mean, std, logprob, n, GaussTail<false>{chw});
  else
    hipLaunchKernelGGL((ddim_step_k<true, false>), ew_grid(n), 256, 0, (hipStream_t)stream, pred, pred_uncond, guidance, xt, noise, t,
                       tables, T, DL_MEAN_V, no_coefs, clamp_x, eta, x_prev, x0_est, mean, std, logprob, n, GaussTail<false>{chw});
  DL_LAUNCH_CHECK();
  return DL_OK;
}

// ---------------------------------------------------------------- guided sampling: CFG rescale, dynamic thresholding
// The Gaussian steps with the two per-sample arrays of the GD kernels above.  One entry point per sampler covers every mean_type (v
// included) and var_mode (DL_VAR_FIXED: [B, chw] prediction; learned: [B, 2 chw] read in place), with the tables of the entry point it
// stands for.  With both arrays NULL the launch is the one dl_ddpm_step / _lv / _v (dl_ddim_step / _lv / _v) makes.
static int step_g_check(const char* who, const void* pred, const void* xt, const void* noise, const void* t, const void* tables,
                        const void* x_prev, int32_t T, int mean_type, int var_mode, int64_t batch, int64_t chw) {
  DL_CHECK_ARG(pred && xt && noise && t && tables && x_prev && batch > 0 && chw > 0 && T > 0, "%s: bad args", who);
  DL_CHECK_ARG(mean_type >= DL_MEAN_EPSILON && mean_type <= DL_MEAN_V, "%s: mean_type %d", who, mean_type);
  DL_CHECK_ARG(var_mode == DL_VAR_FIXED || var_mode == DL_VAR_LEARNED || var_mode == DL_VAR_LEARNED_RANGE, "%s: var_mode %d", who,
               var_mode);
  return DL_OK;
}
extern "C" int dl_ddpm_step_g(const float* pred, const float* pred_uncond, float guidance, const float* cfg_mul, const float* x0_thr,
                              const float* xt, const float* noise, const int32_t* t, const float* tables, int32_t T, int mean_type,
                              int var_mode, int clamp_x, float* x_prev, float* x0_est, float* mean, float* std, float* logprob,
                              int64_t batch, int64_t chw, dl_stream_t stream) {
  if (int rc = step_g_check("dl_ddpm_step_g", pred, xt, noise, t, tables, x_prev, T, mean_type, var_mode, batch, chw)) return rc;
  const int64_t n = batch * chw;
  const bool gd = cfg_mul || x0_thr;
  const GaussTail<true> on{chw, cfg_mul, x0_thr};
  const GaussTail<false> off{chw};
#define DDPM_G(K, TAIL)                                                                                                             \
  hipLaunchKernelGGL(K, ew_grid(n), 256, 0, (hipStream_t)stream, pred, pred_uncond, guidance, xt, noise, t, tables, T, mean_type, \
                     clamp_x, x_prev, x0_est, mean, std, logprob, n, TAIL)
#define DDPM_LV_G(K, TAIL)                                                                                                           \
  hipLaunchKernelGGL(K, ew_grid(n), 256, 0, (hipStream_t)stream, pred, pred_uncond, guidance, xt, noise, t, tables, T, mean_type, \
                     var_mode, clamp_x, x_prev, x0_est, mean, std, logprob, n, TAIL)
  if (var_mode == DL_VAR_FIXED) {
    if (gd) DDPM_G(ddpm_step_k<true>, on); else DDPM_G(ddpm_step_k<false>, off);
  } else {
    if (gd) DDPM_LV_G(ddpm_step_lv_k<true>, on); else DDPM_LV_G(ddpm_step_lv_k<false>, off);
  }
#undef DDPM_G
#undef DDPM_LV_G
  DL_LAUNCH_CHECK();
  return DL_OK;
}
extern "C" int dl_ddim_step_g(const float* pred, const float* pred_uncond, float guidance, const float* cfg_mul, const float* x0_thr,
                              const float* xt, const float* noise, const int32_t* t, const float* tables, int32_t T, int mean_type,
                              int var_mode, const float* ddpm_coefs, int clamp_x, float eta, float* x_prev, float* x0_est,
                              float* mean, float* std, float* logprob, int64_t batch, int64_t chw, dl_stream_t stream) {
  if (int rc = step_g_check("dl_ddim_step_g", pred, xt, noise, t, tables, x_prev, T, mean_type, var_mode, batch, chw)) return rc;
  DL_CHECK_ARG(mean_type != DL_MEAN_XPREV || ddpm_coefs, "dl_ddim_step_g: xprev needs ddpm_coefs");
  const int64_t n = batch * chw;
  const bool gd = cfg_mul || x0_thr;
  const GaussTail<true> on{chw, cfg_mul, x0_thr};
  const GaussTail<false> off{chw};
#define DDIM_G(H, G, TAIL)                                                                                                            \
  hipLaunchKernelGGL((ddim_step_k<H, G>), ew_grid(n), 256, 0, (hipStream_t)stream, pred, pred_uncond, guidance, xt, noise, t, tables, \
                     T, mean_type, ddpm_coefs, clamp_x, eta, x_prev, x0_est, mean, std, logprob, n, TAIL)
  if (var_mode == DL_VAR_FIXED) {
    if (gd) DDIM_G(false, true, on); else DDIM_G(false, false, off);
  } else {
    if (gd) DDIM_G(true, true, on); else DDIM_G(true, false, off);
  }
#undef DDIM_G
  DL_LAUNCH_CHECK();
  return DL_OK;
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

// ---------------------------------------------------------------- hybrid loss of a learned-variance model
// L_simple + L_vlb of Nichol & Dhariwal, "Improved Denoising Diffusion Probabilistic Models" (2021), eq. 16, which the reference
// announces and leaves unwritten (gaussian_diffusion.py:267).  One element's variational-bound term in nats and, where GRAD, its
// derivative with respect to the raw variance output v.  The predicted mean m_p is a constant of that term (the paper's stop-gradient):
// nothing flows into the mean output from here.  tab as in ddpm_step_lv_k.
#define VLB_SQRT_2_OVER_PI 0.7978845608028654f
__device__ __forceinline__ float approx_cdf(float z, float* dz) {  // 0.5 (1 + tanh(sqrt(2/pi) (z + 0.044715 z^3))) and its derivative
  const float th = tanhf(VLB_SQRT_2_OVER_PI * (z + 0.044715f * z * z * z));
  if (dz) *dz = 0.5f * (1.0f - th * th) * VLB_SQRT_2_OVER_PI * (1.0f + 3.0f * 0.044715f * z * z);
  return 0.5f * (1.0f + th);
}
// CLAMP (the evaluation kernel below): the predicted x0 is clamped to [-1, 1] before m_p is formed, and x0_pred, where given,
// receives the x0 the term was formed from.  The training kernels take neither and keep their code.
// DMEAN (the row head's backward for loss_type "vlb", below): no stop-gradient; *dterm_do receives the term's derivative with respect
// to the mean output o, d term / d m_p * d m_p / d o.
template <bool GRAD, bool CLAMP = false, bool DMEAN = false>
__device__ __forceinline__ float vlb_elem(int mean_type, int var_mode, int32_t ti, float o, float v, float x0, float x, float sab,
                                          float ab, float c1, float c2, float lv_q, float beta, float* dterm_dv,
                                          float* x0_pred = nullptr, float* dterm_do = nullptr) {
  float xs = x_start_from(mean_type, o, x, sab, ab, c1, c2);
  if (CLAMP) xs = fminf(fmaxf(xs, -1.0f), 1.0f);
  if (x0_pred) *x0_pred = xs;
  const float m_p = c1 * xs + c2 * x;  // no clamp unless CLAMP
  const float lv_p = learned_log_var(var_mode, v, lv_q, beta);
  float term, dlv, dm = 0.f;  // dm = d term / d m_p (DMEAN)
  if (ti > 0) {  // KL(q(x_{t-1} | x_t, x_0) || p(x_{t-1} | x_t))
    const float d = c1 * x0 + c2 * x - m_p;
    const float r = expf(lv_q - lv_p), q = d * d * expf(-lv_p);
    term = 0.5f * (-1.0f + lv_p - lv_q + r + q);
    dlv = 0.5f * (1.0f - r - q);
    if (DMEAN) dm = -d * expf(-lv_p);
  } else {  // -log of the discretised Gaussian likelihood of x0 (bins of width 2/255), log_scale = lv_p / 2
    const float c = x0 - m_p, s = expf(-0.5f * lv_p);
    const float zp = s * (c + 1.0f / 255.0f), zm = s * (c - 1.0f / 255.0f);
    float dP = 0.f, dQ = 0.f;
    const float P = approx_cdf(zp, (GRAD || DMEAN) ? &dP : nullptr), Q = approx_cdf(zm, (GRAD || DMEAN) ? &dQ : nullptr);
    // d z / d lv_p = -z / 2;  a clamped max(., 1e-12) passes no gradient (torch.clamp)
    float prob, dprob;
    if (x0 < -0.999f) prob = P, dprob = dP * (-0.5f * zp);
    else if (x0 > 0.999f) prob = 1.0f - Q, dprob = -dQ * (-0.5f * zm);
    else prob = P - Q, dprob = dP * (-0.5f * zp) - dQ * (-0.5f * zm);
    term = -logf(fmaxf(prob, 1e-12f));
    dlv = prob > 1e-12f ? -dprob / prob : 0.0f;
    if (DMEAN) {  // d z / d m_p = -s for both CDF arguments; the same clamp rule
      const float dpm = x0 < -0.999f ? dP * -s : (x0 > 0.999f ? dQ * s : (dP - dQ) * -s);
      dm = prob > 1e-12f ? -dpm / prob : 0.0f;
    }
  }
  if (GRAD) *dterm_dv = dlv * (var_mode == DL_VAR_LEARNED ? 1.0f : 0.5f * (logf(beta) - lv_q));
  if (DMEAN) {  // d m_p / d o = c1 d x0_pred / d o (x_start_from)
    float dmo = c1;                                                                // xstart
    if (mean_type == DL_MEAN_EPSILON) dmo = -c1 * (sqrtf(1.0f - ab) / sab);  // = -c1 sqrt(1 / ab - 1), as x_start_from scales o
    else if (mean_type == DL_MEAN_XPREV) dmo = 1.0f;
    else if (mean_type == DL_MEAN_V) dmo = -c1 * sqrtf(1.0f - ab);
    *dterm_do = dm * dmo;
  }
  return term;
}
// partial[blk] = sum (eps - o)^2 and partial[np + blk] = sum of the bound terms over the block's MSE_ELEMS_PER_BLOCK elements, in the
// element-to-thread order of mse_partial_k (the first sum is bit for bit that kernel's on the mean half)
__global__ void vlb_partial_k(const float* __restrict__ pred, const float* __restrict__ eps, const float* __restrict__ x0,
                              const float* __restrict__ xt, const int32_t* __restrict__ t, const float* __restrict__ tab, int32_t T,
                              int mean_type, int var_mode, float* __restrict__ partial, int64_t np, int64_t n, int64_t chw) {
  __shared__ float red[2][MSE_BLOCK / DL_WAVE];
  const int64_t base = (int64_t)blockIdx.x * MSE_ELEMS_PER_BLOCK;
  float acc = 0.f, vacc = 0.f;
#pragma unroll 4
  for (int j = 0; j < 16; ++j) {
    const int64_t i = base + (int64_t)j * MSE_BLOCK + threadIdx.x;
    if (i < n) {
      const int64_t b = i / chw, pi = i + b * chw;
      const int32_t ti = t[b];
      const float o = pred[pi];
      const float d = eps[i] - o;
      acc += d * d;
      vacc += vlb_elem<false>(mean_type, var_mode, ti, o, pred[pi + chw], x0[i], xt[i], tab[ti], tab[T + ti], tab[2 * T + ti],
                              tab[3 * T + ti], tab[4 * T + ti], tab[5 * T + ti], nullptr);
    }
  }
  acc = wave_sum(acc);
  vacc = wave_sum(vacc);
  if ((threadIdx.x & 63) == 0) red[0][threadIdx.x >> 6] = acc, red[1][threadIdx.x >> 6] = vacc;
  __syncthreads();
  if (threadIdx.x < 2) {
    float s = 0.f;
    for (int w = 0; w < MSE_BLOCK / DL_WAVE; ++w) s += red[threadIdx.x][w];
    partial[threadIdx.x * np + blockIdx.x] = s;
  }
}
__global__ void vlb_final_k(const float* __restrict__ partial, float* __restrict__ loss, int64_t np, float inv_n, float inv_n_ln2) {
  __shared__ float red[2][256 / DL_WAVE];
  float acc = 0.f, vacc = 0.f;
  for (int64_t i = threadIdx.x; i < np; i += 256) acc += partial[i], vacc += partial[np + i];
  acc = wave_sum(acc);
  vacc = wave_sum(vacc);
  if ((threadIdx.x & 63) == 0) red[0][threadIdx.x >> 6] = acc, red[1][threadIdx.x >> 6] = vacc;
  __syncthreads();
  if (threadIdx.x < 2)
    loss[threadIdx.x] = (red[threadIdx.x][0] + red[threadIdx.x][1] + red[threadIdx.x][2] + red[threadIdx.x][3]) * (threadIdx.x ? inv_n_ln2 : inv_n);
}
static int vlb_check(const char* who, const void* pred, const void* eps, const void* x0, const void* xt, const void* t,
                     const void* tables, int32_t T, int mean_type, int var_mode, int64_t batch, int64_t chw) {
  DL_CHECK_ARG(pred && eps && x0 && xt && t && tables && batch > 0 && chw > 0 && T > 0, "%s: bad args", who);
  DL_CHECK_ARG(mean_type >= 0 && mean_type <= 2, "%s: mean_type %d", who, mean_type);
  DL_CHECK_ARG(var_mode == DL_VAR_LEARNED || var_mode == DL_VAR_LEARNED_RANGE, "%s: var_mode %d", who, var_mode);
  return DL_OK;
}
extern "C" int dl_vlb_loss_fwd(const float* pred, const float* eps, const float* x0, const float* xt, const int32_t* t,
                               const float* tables, int32_t T, int mean_type, int var_mode, float* partial, float* loss,
                               int64_t batch, int64_t chw, dl_stream_t stream) {
  if (int rc = vlb_check("dl_vlb_loss_fwd", pred, eps, x0, xt, t, tables, T, mean_type, var_mode, batch, chw)) return rc;
  DL_CHECK_ARG(partial && loss, "dl_vlb_loss_fwd: bad args (partial, loss)");
  const int64_t n = batch * chw, np = dl_mse_loss_partials(n);
  hipLaunchKernelGGL(vlb_partial_k, (int)np, MSE_BLOCK, 0, (hipStream_t)stream, pred, eps, x0, xt, t, tables, T, mean_type, var_mode,
                     partial, np, n, chw);
  hipLaunchKernelGGL(vlb_final_k, 1, 256, 0, (hipStream_t)stream, partial, loss, np, (float)(1.0 / (double)n),
                     (float)(1.0 / ((double)n * 0.6931471805599453)));
  DL_LAUNCH_CHECK();
  return DL_OK;
}
__global__ void vlb_bwd_k(const float* __restrict__ pred, const float* __restrict__ eps, const float* __restrict__ x0,
                          const float* __restrict__ xt, const int32_t* __restrict__ t, const float* __restrict__ tab, int32_t T,
                          int mean_type, int var_mode, float coef_m, float coef_v, const float* __restrict__ g_mse,
                          const float* __restrict__ g_vb, float* __restrict__ dpred, int64_t n, int64_t chw) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  if (g_mse) coef_m *= *g_mse;  // as mse_bwd_k forms its coefficient: the mean half is that kernel's output bit for bit
  if (g_vb) coef_v *= *g_vb;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const int64_t b = i / chw, pi = i + b * chw;
    const int32_t ti = t[b];
    const float o = pred[pi];
    float dv;
    vlb_elem<true>(mean_type, var_mode, ti, o, pred[pi + chw], x0[i], xt[i], tab[ti], tab[T + ti], tab[2 * T + ti], tab[3 * T + ti],
                   tab[4 * T + ti], tab[5 * T + ti], &dv);
    dpred[pi] = coef_m * (o - eps[i]);
    dpred[pi + chw] = coef_v * dv;
  }
}
extern "C" int dl_vlb_loss_bwd(const float* pred, const float* eps, const float* x0, const float* xt, const int32_t* t,
                               const float* tables, int32_t T, int mean_type, int var_mode, const float* g_mse_dev,
                               const float* g_vb_dev, float* dpred, int64_t batch, int64_t chw, dl_stream_t stream) {
  if (int rc = vlb_check("dl_vlb_loss_bwd", pred, eps, x0, xt, t, tables, T, mean_type, var_mode, batch, chw)) return rc;
  DL_CHECK_ARG(dpred, "dl_vlb_loss_bwd: bad args (dpred)");
  const int64_t n = batch * chw;
  hipLaunchKernelGGL(vlb_bwd_k, ew_grid(n), 256, 0, (hipStream_t)stream, pred, eps, x0, xt, t, tables, T, mean_type, var_mode,
                     (float)(2.0 / (double)n), (float)(1.0 / ((double)n * 0.6931471805599453)), g_mse_dev, g_vb_dev, dpred, n, chw);
  DL_LAUNCH_CHECK();
  return DL_OK;
}

// ---------------------------------------------------------------- loss head of every parameterisation
// dl_mse_loss_* (mode EPS) and dl_vlb_loss_* generalised: the regression target of the mean output is formed per element from eps,
// x0, xt (never written to memory), the squared error may carry a per-timestep weight, and the prediction is [B, chw] (LV false) or
// [B, 2 chw] with the variational bound on its variance half (LV true).  Only what the mode needs is loaded: the epsilon target
// with fixed variances and no weight reads pred and eps alone, as mse_partial_k does.
// Both are rounded in one defined way (no contraction): the posterior mean as ddpm_step_k rounds its `mean` output, fma(c2, xt, c1 x0),
// and v as two products and a difference, which is also how an f32 host evaluation rounds it.
__device__ __forceinline__ float gd_target(int target, float e, float x0, float x, float sab, float ab, float c1, float c2) {
#pragma clang fp contract(off)
  if (target == DL_MEAN_EPSILON) return e;
  if (target == DL_MEAN_XSTART) return x0;
  if (target == DL_MEAN_XPREV) return __builtin_fmaf(c2, x, c1 * x0);  // ddpm.py:156-174, the posterior mean of (x0, xt)
  return sab * e - sqrtf(1.0f - ab) * x0;  // v; sqrtf(1 - ab) as ddpm_add_noise_k and x_start_from evaluate it
}
__device__ __forceinline__ float gd_sub(float a, float b) {  // a - b, never fused into the arithmetic that formed a
#pragma clang fp contract(off)
  return a - b;
}
struct gd_elem {
  int32_t ti;
  int64_t pi;
  float o, tgt, x0, x, sab, ab, c1, c2;
};
// TI (the row head below, whose per-sample factors are looked up by timestep in every mode): ti is loaded whatever the mode reads
template <bool LV, bool W, bool TI = false>
__device__ __forceinline__ gd_elem gd_load(int64_t i, const float* __restrict__ pred, const float* __restrict__ eps,
                                           const float* __restrict__ x0, const float* __restrict__ xt,
                                           const int32_t* __restrict__ t, const float* __restrict__ tab, int32_t T, int target,
                                           int64_t chw) {
  gd_elem g;
  const bool rows = LV || target >= DL_MEAN_XPREV;
  g.ti = 0;
  g.pi = i;
  if (rows || W || TI) {
    const int64_t b = i / chw;
    g.ti = t[b];
    if (LV) g.pi = i + b * chw;
  }
  g.o = pred[g.pi];
  const float e = (target == DL_MEAN_EPSILON || target == DL_MEAN_V) ? eps[i] : 0.0f;
  g.x0 = (LV || target != DL_MEAN_EPSILON) ? x0[i] : 0.0f;
  g.x = (LV || target == DL_MEAN_XPREV) ? xt[i] : 0.0f;
  g.sab = g.ab = g.c1 = g.c2 = 0.0f;
  if (rows) g.sab = tab[g.ti], g.ab = tab[T + g.ti], g.c1 = tab[2 * T + g.ti], g.c2 = tab[3 * T + g.ti];
  g.tgt = gd_target(target, e, g.x0, g.x, g.sab, g.ab, g.c1, g.c2);
  return g;
}
// partial[blk] = sum w (target - o)^2 and, LV, partial[np + blk] = sum of the bound terms, in the element-to-thread order of
// mse_partial_k / vlb_partial_k.  W false is w == 1: the sum is then accumulated as those kernels accumulate it (acc += d * d), so
// that the epsilon target reproduces their scalars bit for bit.
template <bool LV, bool W>
__global__ void gd_partial_k(const float* __restrict__ pred, const float* __restrict__ eps, const float* __restrict__ x0,
                             const float* __restrict__ xt, const int32_t* __restrict__ t, const float* __restrict__ tab, int32_t T,
                             int target, const float* __restrict__ weight, int var_mode, float* __restrict__ partial, int64_t np,
                             int64_t n, int64_t chw) {
  __shared__ float red[2][MSE_BLOCK / DL_WAVE];
  const int64_t base = (int64_t)blockIdx.x * MSE_ELEMS_PER_BLOCK;
  float acc = 0.f, vacc = 0.f;
#pragma unroll 4
  for (int j = 0; j < 16; ++j) {
    const int64_t i = base + (int64_t)j * MSE_BLOCK + threadIdx.x;
    if (i < n) {
      const gd_elem g = gd_load<LV, W>(i, pred, eps, x0, xt, t, tab, T, target, chw);
      const float d = gd_sub(g.tgt, g.o);
      if (W)
        acc += weight[g.ti] * (d * d);
      else
        acc += d * d;
      if (LV)
        vacc += vlb_elem<false>(target, var_mode, g.ti, g.o, pred[g.pi + chw], g.x0, g.x, g.sab, g.ab, g.c1, g.c2, tab[4 * T + g.ti],
                                tab[5 * T + g.ti], nullptr);
    }
  }
  acc = wave_sum(acc);
  if (LV) vacc = wave_sum(vacc);
  if ((threadIdx.x & 63) == 0) red[0][threadIdx.x >> 6] = acc, red[1][threadIdx.x >> 6] = vacc;
  __syncthreads();
  if (threadIdx.x < (LV ? 2 : 1)) {
    float s = 0.f;
    for (int w = 0; w < MSE_BLOCK / DL_WAVE; ++w) s += red[threadIdx.x][w];
    partial[threadIdx.x * np + blockIdx.x] = s;
  }
}
template <bool LV, bool W>
__global__ void gd_bwd_k(const float* __restrict__ pred, const float* __restrict__ eps, const float* __restrict__ x0,
                         const float* __restrict__ xt, const int32_t* __restrict__ t, const float* __restrict__ tab, int32_t T,
                         int target, const float* __restrict__ weight, int var_mode, float coef_m, float coef_v,
                         const float* __restrict__ g_mse, const float* __restrict__ g_vb, float* __restrict__ dpred, int64_t n,
                         int64_t chw) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  if (g_mse) coef_m *= *g_mse;  // as mse_bwd_k / vlb_bwd_k form their coefficient
  if (LV && g_vb) coef_v *= *g_vb;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const gd_elem g = gd_load<LV, W>(i, pred, eps, x0, xt, t, tab, T, target, chw);
    const float cm = W ? coef_m * weight[g.ti] : coef_m;
    dpred[g.pi] = cm * gd_sub(g.o, g.tgt);
    if (LV) {
      float dv;
      vlb_elem<true>(target, var_mode, g.ti, g.o, pred[g.pi + chw], g.x0, g.x, g.sab, g.ab, g.c1, g.c2, tab[4 * T + g.ti],
                     tab[5 * T + g.ti], &dv);
      dpred[g.pi + chw] = coef_v * dv;
    }
  }
}
static int gd_check(const char* who, const void* pred, const void* eps, const void* x0, const void* xt, const void* t,
                    const void* tables, int32_t T, int target, int var_mode, int64_t batch, int64_t chw) {
  DL_CHECK_ARG(pred && t && tables && batch > 0 && chw > 0 && T > 0, "%s: bad args", who);
  DL_CHECK_ARG(target >= DL_MEAN_EPSILON && target <= DL_MEAN_V, "%s: target %d", who, target);
  DL_CHECK_ARG(var_mode == DL_VAR_FIXED || var_mode == DL_VAR_LEARNED || var_mode == DL_VAR_LEARNED_RANGE, "%s: var_mode %d", who,
               var_mode);
  const bool lv = var_mode != DL_VAR_FIXED;
  DL_CHECK_ARG(eps || target == DL_MEAN_XSTART || target == DL_MEAN_XPREV, "%s: target %d needs eps", who, target);
  DL_CHECK_ARG(x0 || (!lv && target == DL_MEAN_EPSILON), "%s: target %d, var_mode %d need x0", who, target, var_mode);
  DL_CHECK_ARG(xt || (!lv && target != DL_MEAN_XPREV), "%s: target %d, var_mode %d need xt", who, target, var_mode);
  return DL_OK;
}
extern "C" int dl_gd_loss_fwd(const float* pred, const float* eps, const float* x0, const float* xt, const int32_t* t,
                              const float* tables, int32_t T, int target, const float* weight, int var_mode, float* partial,
                              float* loss, int64_t batch, int64_t chw, dl_stream_t stream) {
  if (int rc = gd_check("dl_gd_loss_fwd", pred, eps, x0, xt, t, tables, T, target, var_mode, batch, chw)) return rc;
  DL_CHECK_ARG(partial && loss, "dl_gd_loss_fwd: bad args (partial, loss)");
  const int64_t n = batch * chw, np = dl_mse_loss_partials(n);
  const bool lv = var_mode != DL_VAR_FIXED;
#define GD_FWD(LV, W)                                                                                                            \
  hipLaunchKernelGGL((gd_partial_k<LV, W>), (int)np, MSE_BLOCK, 0, (hipStream_t)stream, pred, eps, x0, xt, t, tables, T, target, \
                     weight, var_mode, partial, np, n, chw)
  if (lv) {
    if (weight) GD_FWD(true, true); else GD_FWD(true, false);
    hipLaunchKernelGGL(vlb_final_k, 1, 256, 0, (hipStream_t)stream, partial, loss, np, (float)(1.0 / (double)n),
                       (float)(1.0 / ((double)n * 0.6931471805599453)));
  } else {
    if (weight) GD_FWD(false, true); else GD_FWD(false, false);
    hipLaunchKernelGGL(mse_final_k, 1, 256, 0, (hipStream_t)stream, partial, loss, np, (float)(1.0 / (double)n));
  }
#undef GD_FWD
  DL_LAUNCH_CHECK();
  return DL_OK;
}
extern "C" int dl_gd_loss_bwd(const float* pred, const float* eps, const float* x0, const float* xt, const int32_t* t,
                              const float* tables, int32_t T, int target, const float* weight, int var_mode,
                              const float* g_mse_dev, const float* g_vb_dev, float* dpred, int64_t batch, int64_t chw,
                              dl_stream_t stream) {
  if (int rc = gd_check("dl_gd_loss_bwd", pred, eps, x0, xt, t, tables, T, target, var_mode, batch, chw)) return rc;
  DL_CHECK_ARG(dpred, "dl_gd_loss_bwd: bad args (dpred)");
  const int64_t n = batch * chw;
  const bool lv = var_mode != DL_VAR_FIXED;
  const float coef_m = (float)(2.0 / (double)n), coef_v = (float)(1.0 / ((double)n * 0.6931471805599453));
#define GD_BWD(LV, W)                                                                                                              \
  hipLaunchKernelGGL((gd_bwd_k<LV, W>), ew_grid(n), 256, 0, (hipStream_t)stream, pred, eps, x0, xt, t, tables, T, target, weight, \
                     var_mode, coef_m, coef_v, g_mse_dev, g_vb_dev, dpred, n, chw)
  if (lv) {
    if (weight) GD_BWD(true, true); else GD_BWD(true, false);
  } else {
    if (weight) GD_BWD(false, true); else GD_BWD(false, false);
  }
#undef GD_BWD
  DL_LAUNCH_CHECK();
  return DL_OK;
}

// ---------------------------------------------------------------- variational bound per (sample, timestep): evaluation
// calc_bpd_loop of Nichol & Dhariwal (2021): what vlb_partial_k sums over the whole batch, kept per row, for fixed variances too, next
// to the two squared errors that loop reports.  A row's chw elements are cut into shares of MSE_ELEMS_PER_BLOCK, one workgroup each,
// walked in the element-to-thread order of mse_partial_k; a row of one share is finished by its workgroup, a longer one leaves its
// share sums in `partial` ([N][rows][nshare]) for rows_final_k, which adds them in share order.  No atomics: every run gives the
// same bits.
template <int N>
struct RowOut {
  float* out[N];
  float scale[N];
};
template <int N>
__device__ __forceinline__ void row_share_finish(float (&acc)[N], float (*red)[MSE_BLOCK / DL_WAVE], const RowOut<N>& ro,
                                                 float* __restrict__ partial, int64_t rows, int64_t row, int64_t nshare,
                                                 int64_t share) {
#pragma unroll
  for (int k = 0; k < N; ++k) acc[k] = wave_sum(acc[k]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < N; ++k) red[k][threadIdx.x >> 6] = acc[k];
  }
  __syncthreads();
  if (threadIdx.x < N) {
    const int k = threadIdx.x;
    float s = 0.f;
    for (int w = 0; w < MSE_BLOCK / DL_WAVE; ++w) s += red[k][w];
    if (nshare == 1)
      ro.out[k][row] = s * ro.scale[k];
    else
      partial[((int64_t)k * rows + row) * nshare + share] = s;
  }
}
template <int N>
__global__ void rows_final_k(const float* __restrict__ partial, const RowOut<N> ro, int64_t rows, int64_t nshare) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // (array k, row)
  if (idx >= N * rows) return;
  const float* p = partial + idx * nshare;
  float s = 0.f;
  for (int64_t j = 0; j < nshare; ++j) s += p[j];
  const int k = (int)(idx / rows);
  ro.out[k][idx - k * rows] = s * ro.scale[k];
}
// LV: pred is [rows, 2 chw] and its variance half gives lv_p by var_mode; else pred is [rows, chw] and lv_p = tab row 5 (the sampler's
// log_variance), handed to vlb_elem as a DL_VAR_LEARNED output.  lv_q = lvq[t] either way (the learned table's row 4 holds the same).
template <bool LV, bool CLAMP>
__global__ void vb_terms_k(const float* __restrict__ pred, const float* __restrict__ eps, const float* __restrict__ x0,
                           const float* __restrict__ xt, const int32_t* __restrict__ t, const float* __restrict__ tab, int32_t T,
                           const float* __restrict__ lvq, int mean_type, int var_mode, float* __restrict__ partial,
                           const RowOut<3> ro, int64_t rows, int64_t chw, int64_t nshare) {
  __shared__ float red[3][MSE_BLOCK / DL_WAVE];
  const int64_t row = blockIdx.x / nshare, share = blockIdx.x - row * nshare;
  const int32_t ti = t[row];
  const float sab = tab[ti], ab = tab[T + ti], c1 = tab[2 * T + ti], c2 = tab[3 * T + ti], r5 = tab[5 * T + ti], lv_q = lvq[ti];
  const float rsab = 1.0f / sab, rden = sqrtf(1.0f / ab - 1.0f);  // eps from x0 as ddim_step_k forms it (ddpm.py:324-326)
  const float* pr = pred + row * (LV ? 2 : 1) * chw;
  const int64_t ro0 = row * chw, base = share * MSE_ELEMS_PER_BLOCK;
  float acc[3] = {0.f, 0.f, 0.f};  // bound term, (x0 - x0_pred)^2, (eps - eps_pred)^2
#pragma unroll 4
  for (int j = 0; j < 16; ++j) {
    const int64_t i = base + (int64_t)j * MSE_BLOCK + threadIdx.x;
    if (i < chw) {
      const float o = pr[i], v = LV ? pr[chw + i] : r5;
      const float xs = x0[ro0 + i], x = xt[ro0 + i];
      float x0p;
      acc[0] += vlb_elem<false, CLAMP>(mean_type, LV ? var_mode : DL_VAR_LEARNED, ti, o, v, xs, x, sab, ab, c1, c2, lv_q, r5, nullptr,
                                       &x0p);
      const float dx = xs - x0p, de = eps[ro0 + i] - (rsab * x - x0p) / rden;
      acc[1] += dx * dx;
      acc[2] += de * de;
    }
  }
  row_share_finish<3>(acc, red, ro, partial, rows, row, nshare, share);
}
extern "C" int dl_vb_terms(const float* pred, const float* eps, const float* x0, const float* xt, const int32_t* t,
                           const float* tables, int32_t T, const float* lv_q, int mean_type, int var_mode, int clip_denoised,
                           float* partial, float* vb, float* xstart_mse, float* mse, int64_t rows, int64_t chw, dl_stream_t stream) {
  DL_CHECK_ARG(pred && eps && x0 && xt && t && tables && lv_q && rows > 0 && chw > 0 && T > 0, "dl_vb_terms: bad args");
  DL_CHECK_ARG(vb && xstart_mse && mse, "dl_vb_terms: bad args (vb, xstart_mse, mse)");
  DL_CHECK_ARG(mean_type >= DL_MEAN_EPSILON && mean_type <= DL_MEAN_V, "dl_vb_terms: mean_type %d", mean_type);
  DL_CHECK_ARG(var_mode == DL_VAR_FIXED || var_mode == DL_VAR_LEARNED || var_mode == DL_VAR_LEARNED_RANGE, "dl_vb_terms: var_mode %d",
               var_mode);
  const int64_t nshare = dl_mse_loss_partials(chw);
  DL_CHECK_ARG(nshare == 1 || partial, "dl_vb_terms: chw %lld needs partial (3 rows dl_mse_loss_partials(chw) floats)", (long long)chw);
  DL_CHECK_ARG(rows <= INT32_MAX / nshare, "dl_vb_terms: rows %lld x %lld shares exceed the grid", (long long)rows, (long long)nshare);
  const float inv = (float)(1.0 / (double)chw);
  const RowOut<3> ro = {{vb, xstart_mse, mse}, {(float)(1.0 / ((double)chw * 0.6931471805599453)), inv, inv}};
  const bool lv = var_mode != DL_VAR_FIXED;
#define VB_TERMS(LV, CLAMP)                                                                                                    \
  hipLaunchKernelGGL((vb_terms_k<LV, CLAMP>), (int)(rows * nshare), MSE_BLOCK, 0, (hipStream_t)stream, pred, eps, x0, xt, t, tables, \
                     T, lv_q, mean_type, var_mode, partial, ro, rows, chw, nshare)
  if (lv) {
    if (clip_denoised) VB_TERMS(true, true); else VB_TERMS(true, false);
  } else {
    if (clip_denoised) VB_TERMS(false, true); else VB_TERMS(false, false);
  }
#undef VB_TERMS
  if (nshare > 1)
    hipLaunchKernelGGL(rows_final_k<3>, cdiv(3 * rows, 256), 256, 0, (hipStream_t)stream, partial, ro, rows, nshare);
  DL_LAUNCH_CHECK();
  return DL_OK;
}
// KL(q(x_T | x0) || N(0, I)) per row in bits per dimension: the mean of 0.5 (-1 - l + exp(l) + ab x0^2), l = log(1 - ab)
__global__ void prior_bpd_k(const float* __restrict__ x0, float ab, float l, float* __restrict__ partial, const RowOut<1> ro,
                            int64_t rows, int64_t chw, int64_t nshare) {
  __shared__ float red[1][MSE_BLOCK / DL_WAVE];
  const int64_t row = blockIdx.x / nshare, share = blockIdx.x - row * nshare;
  const int64_t ro0 = row * chw, base = share * MSE_ELEMS_PER_BLOCK;
  const float c0 = expm1f(l) - l;  // -1 - l + exp(l) without its cancellation (l is about -4e-5 on the 1000-step linear chain)
  float acc[1] = {0.f};
#pragma unroll 4
  for (int j = 0; j < 16; ++j) {
    const int64_t i = base + (int64_t)j * MSE_BLOCK + threadIdx.x;
    if (i < chw) {
      const float x = x0[ro0 + i];
      acc[0] += 0.5f * (c0 + ab * (x * x));
    }
  }
  row_share_finish<1>(acc, red, ro, partial, rows, row, nshare, share);
}
extern "C" int dl_prior_bpd(const float* x0, float alphas_bar_last, float log_one_minus_ab, float* partial, float* out, int64_t batch,
                            int64_t chw, dl_stream_t stream) {
  DL_CHECK_ARG(x0 && out && batch > 0 && chw > 0, "dl_prior_bpd: bad args");
  DL_CHECK_ARG(alphas_bar_last > 0.0f && alphas_bar_last < 1.0f && log_one_minus_ab < 0.0f,
               "dl_prior_bpd: alphas_bar %g in (0, 1) and log(1 - alphas_bar) %g < 0 expected", (double)alphas_bar_last,
               (double)log_one_minus_ab);
  const int64_t nshare = dl_mse_loss_partials(chw);
  DL_CHECK_ARG(nshare == 1 || partial, "dl_prior_bpd: chw %lld needs partial (batch dl_mse_loss_partials(chw) floats)", (long long)chw);
  DL_CHECK_ARG(batch <= INT32_MAX / nshare, "dl_prior_bpd: batch %lld x %lld shares exceed the grid", (long long)batch, (long long)nshare);
  const RowOut<1> ro = {{out}, {(float)(1.0 / ((double)chw * 0.6931471805599453))}};
  hipLaunchKernelGGL(prior_bpd_k, (int)(batch * nshare), MSE_BLOCK, 0, (hipStream_t)stream, x0, alphas_bar_last, log_one_minus_ab,
                     partial, ro, batch, chw, nshare);
  if (nshare > 1) hipLaunchKernelGGL(rows_final_k<1>, cdiv(batch, 256), 256, 0, (hipStream_t)stream, partial, ro, batch, nshare);
  DL_LAUNCH_CHECK();
  return DL_OK;
}

// ---------------------------------------------------------------- ODE likelihood of a rectified-flow model (Flow.calc_nll_loop)
// Instantaneous change of variables with Hutchinson's divergence estimate (Grathwohl et al. 2019, FFJORD): one launch per network
// evaluation behind the input-gradient backward.  A row's chw elements are cut into shares and reduced as vb_terms_k reduces them;
// one sum per row, written as out[oidx] = s * scale + add.
__device__ __forceinline__ void row1_share_finish(float acc, float* red, float* __restrict__ partial, float* __restrict__ out,
                                                  int64_t oidx, float scale, float add, int64_t row, int64_t nshare, int64_t share) {
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = 0.f;
    for (int w = 0; w < MSE_BLOCK / DL_WAVE; ++w) s += red[w];
    if (nshare == 1)
      out[oidx] = s * scale + add;
    else
      partial[row * nshare + share] = s;
  }
}
__global__ void rows1_final_k(const float* __restrict__ partial, float* __restrict__ out, int64_t ld, int64_t col, float scale,
                              float add, int64_t rows, int64_t nshare) {
  const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= rows) return;
  const float* p = partial + row * nshare;
  float s = 0.f;
  for (int64_t j = 0; j < nshare; ++j) s += p[j];
  out[row * ld + col] = s * scale + add;
}
// STEP: x_out = x + a v (+ b v0) over the same elements (x_out may be x: every element is read before it is written, by one thread)
template <bool STEP, bool V0>
__global__ void hutchinson_step_k(const float* x, const float* __restrict__ v, const float* __restrict__ v0, float a, float b,
                                  float* x_out, const float* __restrict__ g, const float* __restrict__ eps, float scale,
                                  float* __restrict__ partial, float* __restrict__ out, int64_t ld, int64_t col, int64_t rows,
                                  int64_t chw, int64_t nshare) {
  __shared__ float red[MSE_BLOCK / DL_WAVE];
  const int64_t row = blockIdx.x / nshare, share = blockIdx.x - row * nshare;
  const int64_t ro0 = row * chw, base = share * MSE_ELEMS_PER_BLOCK;
  float acc = 0.f;
#pragma unroll 4
  for (int j = 0; j < 16; ++j) {
    const int64_t i = base + (int64_t)j * MSE_BLOCK + threadIdx.x;
    if (i < chw) {
      acc += g[ro0 + i] * eps[ro0 + i];
      if constexpr (STEP) {
        float y = x[ro0 + i] + a * v[ro0 + i];
        if constexpr (V0) y += b * v0[ro0 + i];
        x_out[ro0 + i] = y;
      }
    }
  }
  row1_share_finish(acc, red, partial, out, row * ld + col, scale, 0.f, row, nshare, share);
}
extern "C" int dl_hutchinson_step(const float* x, const float* v, const float* v0, float a, float b, float* x_out, const float* g,
                                  const float* eps, float scale, float* partial, float* out, int64_t ld, int64_t col, int64_t rows,
                                  int64_t chw, dl_stream_t stream) {
  DL_CHECK_ARG(g && eps && out && rows > 0 && chw > 0, "dl_hutchinson_step: bad args (g, eps, out, rows, chw)");
  DL_CHECK_ARG(ld > 0 && col >= 0 && col < ld, "dl_hutchinson_step: column %lld of a table of width %lld", (long long)col, (long long)ld);
  DL_CHECK_ARG(!x_out || (x && v), "dl_hutchinson_step: x_out needs x and v");
  DL_CHECK_ARG(x_out || !v0, "dl_hutchinson_step: v0 without x_out");
  const int64_t nshare = dl_mse_loss_partials(chw);
  DL_CHECK_ARG(nshare == 1 || partial, "dl_hutchinson_step: chw %lld needs partial (rows dl_mse_loss_partials(chw) floats)", (long long)chw);
  DL_CHECK_ARG(rows <= INT32_MAX / nshare, "dl_hutchinson_step: rows %lld x %lld shares exceed the grid", (long long)rows, (long long)nshare);
#define HUTCH(STEP, V0)                                                                                                          \
  hipLaunchKernelGGL((hutchinson_step_k<STEP, V0>), (int)(rows * nshare), MSE_BLOCK, 0, (hipStream_t)stream, x, v, v0, a, b, x_out, g, \
                     eps, scale, partial, out, ld, col, rows, chw, nshare)
  if (!x_out) HUTCH(false, false); else if (v0) HUTCH(true, true); else HUTCH(true, false);
#undef HUTCH
  if (nshare > 1)
    hipLaunchKernelGGL(rows1_final_k, cdiv(rows, 256), 256, 0, (hipStream_t)stream, partial, out, ld, col, scale, 0.f, rows, nshare);
  DL_LAUNCH_CHECK();
  return DL_OK;
}
// -log N(x; 0, I) per dimension of every row: out[r] = 0.5 mean(x^2) + 0.5 log(2 pi), nats
__global__ void normal_nll_rows_k(const float* __restrict__ x, float* __restrict__ partial, float* __restrict__ out, float scale,
                                  float add, int64_t rows, int64_t chw, int64_t nshare) {
  __shared__ float red[MSE_BLOCK / DL_WAVE];
  const int64_t row = blockIdx.x / nshare, share = blockIdx.x - row * nshare;
  const int64_t ro0 = row * chw, base = share * MSE_ELEMS_PER_BLOCK;
  float acc = 0.f;
#pragma unroll 4
  for (int j = 0; j < 16; ++j) {
    const int64_t i = base + (int64_t)j * MSE_BLOCK + threadIdx.x;
    if (i < chw) {
      const float xv = x[ro0 + i];
      acc += xv * xv;
    }
  }
  row1_share_finish(acc, red, partial, out, row, scale, add, row, nshare, share);
}
extern "C" int dl_normal_nll_rows(const float* x, float* partial, float* out, int64_t rows, int64_t chw, dl_stream_t stream) {
  DL_CHECK_ARG(x && out && rows > 0 && chw > 0, "dl_normal_nll_rows: bad args");
  const int64_t nshare = dl_mse_loss_partials(chw);
  DL_CHECK_ARG(nshare == 1 || partial, "dl_normal_nll_rows: chw %lld needs partial (rows dl_mse_loss_partials(chw) floats)", (long long)chw);
  DL_CHECK_ARG(rows <= INT32_MAX / nshare, "dl_normal_nll_rows: rows %lld x %lld shares exceed the grid", (long long)rows, (long long)nshare);
  const float scale = (float)(0.5 / (double)chw), add = 0.9189385332046727f;  // 0.5 log(2 pi)
  hipLaunchKernelGGL(normal_nll_rows_k, (int)(rows * nshare), MSE_BLOCK, 0, (hipStream_t)stream, x, partial, out, scale, add, rows, chw,
                     nshare);
  if (nshare > 1) hipLaunchKernelGGL(rows1_final_k, cdiv(rows, 256), 256, 0, (hipStream_t)stream, partial, out, (int64_t)1, (int64_t)0, scale, add, rows, nshare);
  DL_LAUNCH_CHECK();
  return DL_OK;
}

// ---------------------------------------------------------------- row head: per-sample losses, L_vlb, loss-aware timestep sampling
// Nichol & Dhariwal (2021), sec. 3.3: training on the bound itself, the timestep drawn by importance from a running second moment
// of the per-timestep loss (`LossSecondMomentResampler` of their code base).  gd_partial_k kept per sample: a row's shares are
// walked and reduced as vb_terms_k does it, the batch scalars are formed from the rows in ascending b by one workgroup.
template <bool LV>
__global__ void gd_rows_k(const float* __restrict__ pred, const float* __restrict__ eps, const float* __restrict__ x0,
                          const float* __restrict__ xt, const int32_t* __restrict__ t, const float* __restrict__ tab, int32_t T,
                          int target, int var_mode, float* __restrict__ partial, const RowOut<(LV ? 2 : 1)> ro, int64_t rows,
                          int64_t chw, int64_t nshare) {
  constexpr int N = LV ? 2 : 1;
  __shared__ float red[N][MSE_BLOCK / DL_WAVE];
  const int64_t row = blockIdx.x / nshare, share = blockIdx.x - row * nshare;
  const int64_t ro0 = row * chw, base = share * MSE_ELEMS_PER_BLOCK;
  float acc[N] = {};  // (target - o)^2, bound term
#pragma unroll 4
  for (int j = 0; j < 16; ++j) {
    const int64_t r = base + (int64_t)j * MSE_BLOCK + threadIdx.x;
    if (r < chw) {
      const gd_elem g = gd_load<LV, false, true>(ro0 + r, pred, eps, x0, xt, t, tab, T, target, chw);
      const float d = gd_sub(g.tgt, g.o);
      acc[0] += d * d;
      if constexpr (LV)
        acc[1] += vlb_elem<false>(target, var_mode, g.ti, g.o, pred[g.pi + chw], g.x0, g.x, g.sab, g.ab, g.c1, g.c2, tab[4 * T + g.ti],
                                  tab[5 * T + g.ti], nullptr);
    }
  }
  row_share_finish<N>(acc, red, ro, partial, rows, row, nshare, share);
}
// one workgroup: finishes the rows of more than one share (share order), forms total_row and the two batch scalars (ascending b:
// 256 rows at a time go through shared memory, thread k sums scalar k)
template <bool LV>
__global__ __launch_bounds__(256) void gd_rows_final_k(const float* __restrict__ partial, const int32_t* __restrict__ t,
                                                       const float* __restrict__ weight, const float* __restrict__ imp,
                                                       float vb_scale, int vlb, const RowOut<(LV ? 2 : 1)> ro,
                                                       float* __restrict__ total_row, float* __restrict__ loss, int64_t rows,
                                                       int64_t nshare, float inv_rows) {
  constexpr int N = LV ? 2 : 1;
  __shared__ float sm[N][256];
  float s = 0.f;
  for (int64_t base = 0; base < rows; base += 256) {
    const int64_t b = base + threadIdx.x;
    float a[2] = {0.f, 0.f};
    if (b < rows) {
      float r[2] = {0.f, 0.f};
#pragma unroll
      for (int k = 0; k < N; ++k) {
        if (nshare == 1) {
          r[k] = ro.out[k][b];
        } else {
          const float* p = partial + ((int64_t)k * rows + b) * nshare;
          float q = 0.f;
          for (int64_t j = 0; j < nshare; ++j) q += p[j];
          r[k] = q * ro.scale[k];
          ro.out[k][b] = r[k];
        }
      }
      const int32_t ti = t[b];
      const float wm = weight ? weight[ti] * r[0] : r[0], im = imp ? imp[ti] : 1.0f;
      total_row[b] = vlb ? r[1] : (LV ? wm + vb_scale * r[1] : wm);
      a[0] = im * wm;
      a[1] = im * r[1];
    }
#pragma unroll
    for (int k = 0; k < N; ++k) sm[k][threadIdx.x] = a[k];
    __syncthreads();
    if (threadIdx.x < N) {
      const int m = (int)(rows - base < 256 ? rows - base : 256);
      for (int k = 0; k < m; ++k) s += sm[threadIdx.x][k];
    }
    __syncthreads();
  }
  if (threadIdx.x < N) loss[threadIdx.x] = s * inv_rows;
}
// gd_bwd_k with the per-sample importance weight and, DMEAN, the bound's derivative into the mean output
template <bool LV, bool W, bool DMEAN>
__global__ void gd_rows_bwd_k(const float* __restrict__ pred, const float* __restrict__ eps, const float* __restrict__ x0,
                              const float* __restrict__ xt, const int32_t* __restrict__ t, const float* __restrict__ tab, int32_t T,
                              int target, const float* __restrict__ weight, const float* __restrict__ imp, int var_mode, float coef_m,
                              float coef_v, const float* __restrict__ g_mse, const float* __restrict__ g_vb,
                              float* __restrict__ dpred, int64_t n, int64_t chw) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  if (g_mse) coef_m *= *g_mse;  // as gd_bwd_k forms its coefficients
  if (LV && g_vb) coef_v *= *g_vb;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const gd_elem g = gd_load<LV, W, true>(i, pred, eps, x0, xt, t, tab, T, target, chw);
    float cm = W ? coef_m * weight[g.ti] : coef_m, cv = coef_v;
    if (imp) {
      const float im = imp[g.ti];
      cm *= im;
      cv *= im;
    }
    float dm = cm * gd_sub(g.o, g.tgt);
    if constexpr (LV) {
      float dv, dvo = 0.f;
      vlb_elem<true, false, DMEAN>(target, var_mode, g.ti, g.o, pred[g.pi + chw], g.x0, g.x, g.sab, g.ab, g.c1, g.c2,
                                   tab[4 * T + g.ti], tab[5 * T + g.ti], &dv, nullptr, &dvo);
      dpred[g.pi + chw] = cv * dv;
      if (DMEAN) dm += cv * dvo;
    }
    dpred[g.pi] = dm;
  }
}
static int gd_rows_check(const char* who, int var_mode, int loss_type) {
  DL_CHECK_ARG(loss_type == DL_LOSS_TYPE_MSE || loss_type == DL_LOSS_TYPE_VLB, "%s: loss_type %d", who, loss_type);
  DL_CHECK_ARG(loss_type == DL_LOSS_TYPE_MSE || var_mode != DL_VAR_FIXED, "%s: DL_LOSS_TYPE_VLB needs learned variances", who);
  return DL_OK;
}
extern "C" int dl_gd_loss_rows_fwd(const float* pred, const float* eps, const float* x0, const float* xt, const int32_t* t,
                                   const float* tables, int32_t T, int target, const float* weight, const float* imp, int var_mode,
                                   int loss_type, float vb_scale, float* partial, float* mse_row, float* vb_row, float* total_row,
                                   float* loss, int64_t batch, int64_t chw, dl_stream_t stream) {
  if (int rc = gd_check("dl_gd_loss_rows_fwd", pred, eps, x0, xt, t, tables, T, target, var_mode, batch, chw)) return rc;
  if (int rc = gd_rows_check("dl_gd_loss_rows_fwd", var_mode, loss_type)) return rc;
  const bool lv = var_mode != DL_VAR_FIXED;
  DL_CHECK_ARG(mse_row && total_row && loss && (vb_row || !lv), "dl_gd_loss_rows_fwd: bad args (mse_row, vb_row, total_row, loss)");
  const int64_t nshare = dl_mse_loss_partials(chw);
  DL_CHECK_ARG(nshare == 1 || partial, "dl_gd_loss_rows_fwd: chw %lld needs partial (2 batch dl_mse_loss_partials(chw) floats)",
               (long long)chw);
  DL_CHECK_ARG(batch <= INT32_MAX / nshare, "dl_gd_loss_rows_fwd: batch %lld x %lld shares exceed the grid", (long long)batch,
               (long long)nshare);
  const float inv = (float)(1.0 / (double)chw), inv_ln2 = (float)(1.0 / ((double)chw * 0.6931471805599453));
  const float inv_b = (float)(1.0 / (double)batch);
  const int vlb = loss_type == DL_LOSS_TYPE_VLB;
  if (lv) {
    const RowOut<2> ro = {{mse_row, vb_row}, {inv, inv_ln2}};
    hipLaunchKernelGGL(gd_rows_k<true>, (int)(batch * nshare), MSE_BLOCK, 0, (hipStream_t)stream, pred, eps, x0, xt, t, tables, T,
                       target, var_mode, partial, ro, batch, chw, nshare);
    hipLaunchKernelGGL(gd_rows_final_k<true>, 1, 256, 0, (hipStream_t)stream, partial, t, weight, imp, vb_scale, vlb, ro, total_row,
                       loss, batch, nshare, inv_b);
  } else {
    const RowOut<1> ro = {{mse_row}, {inv}};
    hipLaunchKernelGGL(gd_rows_k<false>, (int)(batch * nshare), MSE_BLOCK, 0, (hipStream_t)stream, pred, eps, x0, xt, t, tables, T,
                       target, var_mode, partial, ro, batch, chw, nshare);
    hipLaunchKernelGGL(gd_rows_final_k<false>, 1, 256, 0, (hipStream_t)stream, partial, t, weight, imp, vb_scale, vlb, ro, total_row,
                       loss, batch, nshare, inv_b);
  }
  DL_LAUNCH_CHECK();
  return DL_OK;
}
extern "C" int dl_gd_loss_rows_bwd(const float* pred, const float* eps, const float* x0, const float* xt, const int32_t* t,
                                   const float* tables, int32_t T, int target, const float* weight, const float* imp, int var_mode,
                                   int loss_type, const float* g_mse_dev, const float* g_vb_dev, float* dpred, int64_t batch,
                                   int64_t chw, dl_stream_t stream) {
  if (int rc = gd_check("dl_gd_loss_rows_bwd", pred, eps, x0, xt, t, tables, T, target, var_mode, batch, chw)) return rc;
  if (int rc = gd_rows_check("dl_gd_loss_rows_bwd", var_mode, loss_type)) return rc;
  DL_CHECK_ARG(dpred, "dl_gd_loss_rows_bwd: bad args (dpred)");
  const int64_t n = batch * chw;
  const bool lv = var_mode != DL_VAR_FIXED;
  const float coef_m = (float)(2.0 / (double)n), coef_v = (float)(1.0 / ((double)n * 0.6931471805599453));
#define GD_ROWS_BWD(LV, W, DMEAN)                                                                                                \
  hipLaunchKernelGGL((gd_rows_bwd_k<LV, W, DMEAN>), ew_grid(n), 256, 0, (hipStream_t)stream, pred, eps, x0, xt, t, tables, T, target, \
                     weight, imp, var_mode, coef_m, coef_v, g_mse_dev, g_vb_dev, dpred, n, chw)
  if (loss_type == DL_LOSS_TYPE_VLB) {
    if (weight) GD_ROWS_BWD(true, true, true); else GD_ROWS_BWD(true, false, true);
  } else if (lv) {
    if (weight) GD_ROWS_BWD(true, true, false); else GD_ROWS_BWD(true, false, false);
  } else {
    if (weight) GD_ROWS_BWD(false, true, false); else GD_ROWS_BWD(false, false, false);
  }
#undef GD_ROWS_BWD
  DL_LAUNCH_CHECK();
  return DL_OK;
}

// the resampler's state, one launch per training step: one workgroup, thread i owns the histories of timesteps i, i + 1024, ...
#define HIST_THREADS 1024
#define HIST_MAX_T 4096
#define HIST_MAX_N 65536
__global__ __launch_bounds__(HIST_THREADS) void loss_history_update_k(const int32_t* __restrict__ t, const float* __restrict__ loss,
                                                                       int n, float* __restrict__ hist, int32_t* __restrict__ count,
                                                                       float* __restrict__ p, float* __restrict__ imp,
                                                                       float* __restrict__ cdf, int T, int H, float uniform_prob) {
  __shared__ float sp[HIST_MAX_T];
  __shared__ float wsum[HIST_THREADS / DL_WAVE];
  __shared__ __attribute__((aligned(16))) int32_t st[HIST_THREADS];
  __shared__ float sl[HIST_THREADS];
  __shared__ int not_full;
  constexpr int OWN = HIST_MAX_T / HIST_THREADS;
  if (threadIdx.x == 0) not_full = 0;
  // Applying k pairs in order to a row that holds c of its H slots leaves the last min(H, c + k) entries of (old entries, new losses):
  // drop = max(0, c + k - H) entries fall off the front.  So the pairs are walked twice, 1024 at a time through shared memory (four
  // indices compared per read): once to count a thread's pairs, then -- after the kept old entries have moved to the front -- to put
  // the j-th of them at slot c + j - drop.  Array order is kept (chunks ascend, a thread walks a chunk in order), and no work that
  // waits on memory sits in the divergent branch of a match: the lanes of a wave meet their pairs at different iterations, so
  // whatever that branch waits for is waited for one lane after the other.
  int c[OWN], k[OWN], drop[OWN];
#pragma unroll
  for (int q = 0; q < OWN; ++q) {
    const int i = threadIdx.x + q * HIST_THREADS;
    c[q] = i < T ? min(max(count[i], 0), H) : 0;  // (a count from outside this kernel never indexes past the row)
    k[q] = 0;
  }
  for (int j0 = 0; j0 < n; j0 += HIST_THREADS) {
    __syncthreads();
    st[threadIdx.x] = j0 + threadIdx.x < n ? t[j0 + threadIdx.x] : -1;
    __syncthreads();
    const int m = min(HIST_THREADS, n - j0);
#pragma unroll
    for (int q = 0; q < OWN; ++q) {
      const int i = threadIdx.x + q * HIST_THREADS;
      if (i < T)
        for (int jj = 0; jj < m; jj += 4) {
          const int4 v = *reinterpret_cast<const int4*>(&st[jj]);
          k[q] += (v.x == i) + (v.y == i) + (v.z == i) + (v.w == i);
        }
    }
  }
#pragma unroll
  for (int q = 0; q < OWN; ++q) {
    const int i = threadIdx.x + q * HIST_THREADS;
    drop[q] = max(0, c[q] + k[q] - H);
    const int keep = i < T && k[q] > 0 && drop[q] > 0 ? c[q] - drop[q] : 0;  // old entries that stay, moved to slots 0 .. keep-1
    float* h = hist + (int64_t)i * H;
    for (int r0 = 0; r0 < keep; r0 += 8) {  // eight slots per round trip; a slot is read in the round before the one that overwrites it
      float a[8];
#pragma unroll
      for (int r = 0; r < 8; ++r) a[r] = r0 + r < keep ? h[r0 + r + drop[q]] : 0.f;
#pragma unroll
      for (int r = 0; r < 8; ++r)
        if (r0 + r < keep) h[r0 + r] = a[r];
    }
  }
  bool any = false;
#pragma unroll
  for (int q = 0; q < OWN; ++q) any |= k[q] > 0;
  for (int j0 = 0; j0 < n; j0 += HIST_THREADS) {
    __syncthreads();
    const bool in = j0 + threadIdx.x < n;
    st[threadIdx.x] = in ? t[j0 + threadIdx.x] : -1;
    sl[threadIdx.x] = in ? loss[j0 + threadIdx.x] : 0.f;
    __syncthreads();
    if (!any) continue;
    const int m = min(HIST_THREADS, n - j0);
#pragma unroll
    for (int q = 0; q < OWN; ++q) {
      const int i = threadIdx.x + q * HIST_THREADS;
      if (i < T && k[q] > 0) {
        float* h = hist + (int64_t)i * H;
        for (int jj = 0; jj < m; jj += 4) {
          const int4 v = *reinterpret_cast<const int4*>(&st[jj]);
          if (v.x != i && v.y != i && v.z != i && v.w != i) continue;
          const int e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
          for (int k4 = 0; k4 < 4; ++k4) {
            if (e[k4] != i) continue;
            const int pos = c[q] - drop[q];  // c counts up through the pairs: the slot of this one, negative if it falls off too
            if (pos >= 0) h[pos] = sl[jj + k4];
            ++c[q];
          }
        }
      }
    }
  }
#pragma unroll
  for (int q = 0; q < OWN; ++q) c[q] = min(c[q], H);
  float local = 0.f;
  bool nf = false;
#pragma unroll
  for (int q = 0; q < OWN; ++q) {
    const int i = threadIdx.x + q * HIST_THREADS;
    if (i < T) {
      const float* h = hist + (int64_t)i * H;
      count[i] = c[q];
      nf |= c[q] != H;
      float s = 0.f;
      for (int slot = 0; slot < H; ++slot) s += h[slot] * h[slot];
      const float r = sqrtf(s / (float)H);
      sp[i] = r;
      local += r;  // ascending i within the thread
    }
  }
  __syncthreads();  // (not_full = 0 above, where n == 0 met no barrier)
  if (nf) not_full = 1;  // (every writer stores the same value)
  local = wave_sum(local);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = local;
  __syncthreads();
  float total = 0.f;
  for (int w = 0; w < HIST_THREADS / DL_WAVE; ++w) total += wsum[w];
  const bool warm = !not_full && total > 0.0f;
  const float uni = 1.0f / (float)T;
  for (int i = threadIdx.x; i < T; i += HIST_THREADS) {
    const float pi = warm ? sp[i] / total * (1.0f - uniform_prob) + uniform_prob / (float)T : uni;
    sp[i] = pi;
    p[i] = pi;
    imp[i] = 1.0f / ((float)T * pi);
  }
  __syncthreads();
  if (threadIdx.x == 0) {  // a serial prefix sum: ascending order, and non-decreasing whatever the rounding
    float run = 0.f;
    for (int i = 0; i < T; ++i) {
      run += sp[i];
      sp[i] = run;
    }
    sp[T - 1] = 1.0f;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < T; i += HIST_THREADS) cdf[i] = sp[i];
}
extern "C" int dl_loss_history_update(const int32_t* t, const float* loss, int64_t n, float* hist, int32_t* count, float* p,
                                      float* imp, float* cdf, int32_t T, int32_t H, float uniform_prob, dl_stream_t stream) {
  DL_CHECK_ARG(hist && count && p && imp && cdf && T > 0 && H > 0 && n >= 0, "dl_loss_history_update: bad args");
  DL_CHECK_ARG(n == 0 || (t && loss), "dl_loss_history_update: bad args (t, loss with n %lld)", (long long)n);
  DL_CHECK_ARG(uniform_prob >= 0.0f && uniform_prob <= 1.0f, "dl_loss_history_update: uniform_prob %g outside [0, 1]",
               (double)uniform_prob);
  if (T > HIST_MAX_T || n > HIST_MAX_N) {
    dl_set_error("dl_loss_history_update: T %d above %d or n %lld above %d", T, HIST_MAX_T, (long long)n, HIST_MAX_N);
    return DL_ERR_UNSUPPORTED;
  }
  hipLaunchKernelGGL(loss_history_update_k, 1, HIST_THREADS, 0, (hipStream_t)stream, t, loss, (int)n, hist, count, p, imp, cdf, T, H,
                     uniform_prob);
  DL_LAUNCH_CHECK();
  return DL_OK;
}
__global__ void draw_timesteps_k(const float* __restrict__ u, const float* __restrict__ cdf, int T, int32_t* __restrict__ out,
                                 int64_t n) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n) return;
  const float x = u[b];
  int lo = 0, hi = T - 1;  // the first index with cdf > x lies in [lo, hi], or there is none and T - 1 is returned
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (cdf[mid] > x) hi = mid; else lo = mid + 1;
  }
  out[b] = lo;
}
extern "C" int dl_draw_timesteps(const float* u, const float* cdf, int32_t T, int32_t* t_out, int64_t batch, dl_stream_t stream) {
  DL_CHECK_ARG(u && cdf && t_out && T > 0 && batch > 0, "dl_draw_timesteps: bad args");
  DL_CHECK_ARG(batch <= (int64_t)INT32_MAX * 256, "dl_draw_timesteps: batch %lld exceeds the grid", (long long)batch);
  hipLaunchKernelGGL(draw_timesteps_k, cdiv(batch, 256), 256, 0, (hipStream_t)stream, u, cdf, T, t_out, batch);
  DL_LAUNCH_CHECK();
  return DL_OK;
}

// ---------------------------------------------------------------- optimizer / casts
// CLIP: the gradient scale is grad_scale * *coef, the clipping coefficient dl_clip_coef left in device memory (clip.hip); formed once
// per thread, so with *coef == 1 the update is bit-identical to the plain one
template <bool CLIP>
__global__ void adamw_k(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                        float* __restrict__ v, int64_t n4, int64_t n, float lr, float b1, float b2, float eps,
                        float wd, float inv_bc1_lr, float inv_sqrt_bc2, float grad_scale, const float* __restrict__ coef) {
  const float gs = CLIP ? grad_scale * *coef : grad_scale;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    float4 pp = ((float4*)p)[i], gg = ((const float4*)g)[i], mm = ((float4*)m)[i], vv = ((float4*)v)[i];
    float* P = (float*)&pp;
    float* G = (float*)&gg;
    float* Mm = (float*)&mm;
    float* V = (float*)&vv;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float gr = G[j] * gs;
      float pj = P[j] * (1.0f - lr * wd);
      const float mj = b1 * Mm[j] + (1.0f - b1) * gr;
      const float vj = b2 * V[j] + (1.0f - b2) * gr * gr;
      const float denom = sqrtf(vj) * inv_sqrt_bc2 + eps;
      pj -= inv_bc1_lr * (mj / denom);
      P[j] = pj;
      Mm[j] = mj;
      V[j] = vj;
    }
    ((float4*)p)[i] = pp;
    ((float4*)m)[i] = mm;
    ((float4*)v)[i] = vv;
  }
  // tail (n % 4)
  const int64_t tail0 = n4 * 4;
  const int64_t gi = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gi < n - tail0) {
    const int64_t i = tail0 + gi;
    const float gr = g[i] * gs;
    float pj = p[i] * (1.0f - lr * wd);
    const float mj = b1 * m[i] + (1.0f - b1) * gr;
    const float vj = b2 * v[i] + (1.0f - b2) * gr * gr;
    pj -= inv_bc1_lr * (mj / (sqrtf(vj) * inv_sqrt_bc2 + eps));
    p[i] = pj;
    m[i] = mj;
    v[i] = vj;
  }
}
extern "C" int dl_adamw_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1,
                             float beta2, float eps, float weight_decay, float bias_corr1, float bias_corr2,
                             float grad_scale, dl_stream_t stream) {
  DL_CHECK_ARG(p && g && m && v && n > 0, "dl_adamw_step: bad args");
  DL_CHECK_ARG((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0, "dl_adamw_step: 16B alignment");
  const float inv_bc1_lr = (float)((double)lr / (double)bias_corr1);
  const float inv_sqrt_bc2 = (float)(1.0 / sqrt((double)bias_corr2));
  hipLaunchKernelGGL(adamw_k<false>, ew_grid(n / 4 + 1), 256, 0, (hipStream_t)stream, p, g, m, v, n / 4, n, lr, beta1, beta2,
                     eps, weight_decay, inv_bc1_lr, inv_sqrt_bc2, grad_scale, (const float*)nullptr);
  DL_LAUNCH_CHECK();
  return DL_OK;
}
extern "C" int dl_adamw_step_clip(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1,
                                  float beta2, float eps, float weight_decay, float bias_corr1, float bias_corr2,
                                  float grad_scale, const float* coef, dl_stream_t stream) {
  DL_CHECK_ARG(p && g && m && v && coef && n > 0, "dl_adamw_step_clip: bad args");
  DL_CHECK_ARG((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0, "dl_adamw_step_clip: 16B alignment");
  const float inv_bc1_lr = (float)((double)lr / (double)bias_corr1);
  const float inv_sqrt_bc2 = (float)(1.0 / sqrt((double)bias_corr2));
  hipLaunchKernelGGL(adamw_k<true>, ew_grid(n / 4 + 1), 256, 0, (hipStream_t)stream, p, g, m, v, n / 4, n, lr, beta1, beta2,
                     eps, weight_decay, inv_bc1_lr, inv_sqrt_bc2, grad_scale, coef);
  DL_LAUNCH_CHECK();
  return DL_OK;
}

// same update with the scalars read from device memory (hyper = {lr, beta1, beta2, eps, weight_decay, lr / bias_corr1,
// 1 / sqrt(bias_corr2), grad_scale}): the launch carries no per-step value, so a captured hipGraph of the training step can be
// replayed while the host refreshes the 32 bytes before each replay (training/graph_step.py)
// The roundings are written out (contraction off, each fused multiply-add explicit) in the form the plain kernel has always compiled
// to: left to the compiler, the CLIP instantiation fused v's update differently and came out an ulp apart at *coef == 1.
template <bool CLIP>
__global__ void adamw_dev_k(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                            int64_t n, const float* __restrict__ hyper, const float* __restrict__ coef) {
#pragma clang fp contract(off)
  const float lr = hyper[0], b1 = hyper[1], b2 = hyper[2], eps = hyper[3], wd = hyper[4], inv_bc1_lr = hyper[5],
              inv_sqrt_bc2 = hyper[6], gs = CLIP ? hyper[7] * *coef : hyper[7];
  const float decay = __builtin_fmaf(-lr, wd, 1.0f), omb1 = 1.0f - b1, omb2 = 1.0f - b2;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const float gr = g[i] * gs;
    const float mj = __builtin_fmaf(b1, m[i], omb1 * gr);
    const float vj = __builtin_fmaf(gr, omb2 * gr, b2 * v[i]);
    const float denom = __builtin_fmaf(sqrtf(vj), inv_sqrt_bc2, eps);
    p[i] = decay * p[i] - inv_bc1_lr * (mj / denom);
    m[i] = mj;
    v[i] = vj;
  }
}
extern "C" int dl_adamw_step_dev(float* p, const float* g, float* m, float* v, int64_t n, const float* hyper, dl_stream_t stream) {
  DL_CHECK_ARG(p && g && m && v && hyper && n > 0, "dl_adamw_step_dev: bad args");
  hipLaunchKernelGGL(adamw_dev_k<false>, ew_grid(n), 256, 0, (hipStream_t)stream, p, g, m, v, n, hyper, (const float*)nullptr);
  DL_LAUNCH_CHECK();
  return DL_OK;
}
extern "C" int dl_adamw_step_dev_clip(float* p, const float* g, float* m, float* v, int64_t n, const float* hyper, const float* coef,
                                      dl_stream_t stream) {
  DL_CHECK_ARG(p && g && m && v && hyper && coef && n > 0, "dl_adamw_step_dev_clip: bad args");
  hipLaunchKernelGGL(adamw_dev_k<true>, ew_grid(n), 256, 0, (hipStream_t)stream, p, g, m, v, n, hyper, coef);
  DL_LAUNCH_CHECK();
  return DL_OK;
}

// torch.optim.SGD's single-tensor rule for one element.  ONE body for every caller (vector lanes, scalar head / tail, the odd-phase
// loop; scalars from the launch or from device memory; with or without the clipping coefficient), with contraction off and each
// fused multiply-add explicit, as in adamw_dev_k and for its reason: all of them round identically, which the tests hold bit for bit.
struct SgdScalars {
  float neg_lr, mom, omd, wd, gs;  // -lr, momentum, 1 - dampening, weight_decay, grad_scale [* *coef]
  int flags;
  bool has_buf;
};
__device__ __forceinline__ void sgd_elem(float& p, const float g, float& b, const SgdScalars& s) {
#pragma clang fp contract(off)
  float gr = g * s.gs;
  if (s.flags & DL_SGD_MAXIMIZE) gr = -gr;
  if (s.wd != 0.0f) gr = __builtin_fmaf(s.wd, p, gr);
  if (s.has_buf) {
    b = (s.flags & DL_SGD_FIRST) ? gr : __builtin_fmaf(s.mom, b, s.omd * gr);
    gr = (s.flags & DL_SGD_NESTEROV) ? __builtin_fmaf(s.mom, b, gr) : b;
  }
  p = __builtin_fmaf(s.neg_lr, gr, p);
}
// Elements [head, head + 4 * n4) go as float4 (the host picks `head` so that p + head, g + head and buf + head are 16-byte aligned);
// [0, head) and [head + 4 * n4, n) go one by one.  Buffers whose 16-byte phases differ: head = n, n4 = 0, a scalar grid-stride loop.
// buf == NULL: no momentum, the buffer is neither read nor written.  DL_SGD_FIRST writes buf without reading it.
__global__ void sgd_k(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf, int64_t n, int64_t head,
                      int64_t n4, float lr, float mom, float damp, float wd, float grad_scale, const float* __restrict__ hyper,
                      const float* __restrict__ coef, int flags) {
#pragma clang fp contract(off)
  if (hyper) lr = hyper[0], mom = hyper[1], damp = hyper[2], wd = hyper[3], grad_scale = hyper[4];
  SgdScalars s;
  s.neg_lr = -lr, s.mom = mom, s.omd = 1.0f - damp, s.wd = wd, s.gs = coef ? grad_scale * *coef : grad_scale;
  s.flags = flags, s.has_buf = buf != nullptr;
  const bool read_buf = s.has_buf && !(flags & DL_SGD_FIRST);
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
  float4* p4 = (float4*)(p + head);
  const float4* g4 = (const float4*)(g + head);
  float4* b4 = s.has_buf ? (float4*)(buf + head) : nullptr;
  for (int64_t i = tid; i < n4; i += stride) {
    float4 pp = p4[i], bb = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const float4 gg = g4[i];
    if (read_buf) bb = b4[i];
    sgd_elem(pp.x, gg.x, bb.x, s);
    sgd_elem(pp.y, gg.y, bb.y, s);
    sgd_elem(pp.z, gg.z, bb.z, s);
    sgd_elem(pp.w, gg.w, bb.w, s);
    p4[i] = pp;
    if (s.has_buf) b4[i] = bb;
  }
  const int64_t tail0 = head + 4 * n4, n_scalar = head + (n - tail0);
  for (int64_t j = tid; j < n_scalar; j += stride) {
    const int64_t i = j < head ? j : tail0 + (j - head);
    float pj = p[i], bj = read_buf ? buf[i] : 0.0f;
    sgd_elem(pj, g[i], bj, s);
    p[i] = pj;
    if (s.has_buf) buf[i] = bj;
  }
}
static int sgd_launch(const char* who, float* p, const float* g, float* buf, int64_t n, float lr, float mom, float damp, float wd,
                      float grad_scale, const float* hyper, const float* coef, int flags, dl_stream_t stream) {
  DL_CHECK_ARG(p && g && n > 0, "%s: bad args (p, g non-null, n > 0)", who);
  DL_CHECK_ARG(((((uintptr_t)p | (uintptr_t)g | (uintptr_t)buf | (uintptr_t)coef | (uintptr_t)hyper)) & 3) == 0, "%s: 4B alignment", who);
  DL_CHECK_ARG((flags & ~(DL_SGD_NESTEROV | DL_SGD_FIRST | DL_SGD_MAXIMIZE)) == 0, "%s: unknown flag bits 0x%x", who, flags);
  const int ph = (int)(((uintptr_t)p >> 2) & 3);
  const bool same = ph == (int)(((uintptr_t)g >> 2) & 3) && (!buf || ph == (int)(((uintptr_t)buf >> 2) & 3));
  int64_t head = n, n4 = 0;
  if (same) {
    head = (4 - ph) & 3;
    if (head > n) head = n;
    n4 = (n - head) / 4;
  }
  const int64_t n_scalar = n - 4 * n4;
  hipLaunchKernelGGL(sgd_k, ew_grid(n4 > n_scalar ? n4 : n_scalar), 256, 0, (hipStream_t)stream, p, g, buf, n, head, n4, lr, mom,
                     damp, wd, grad_scale, hyper, coef, flags);
  DL_LAUNCH_CHECK();
  return DL_OK;
}
extern "C" int dl_sgd_step(float* p, const float* g, float* buf, int64_t n, float lr, float momentum, float dampening,
                           float weight_decay, float grad_scale, const float* coef, int flags, dl_stream_t stream) {
  DL_CHECK_ARG(momentum == 0.0f || buf, "dl_sgd_step: momentum != 0 needs a momentum buffer");
  DL_CHECK_ARG(!(flags & DL_SGD_NESTEROV) || (momentum != 0.0f && dampening == 0.0f),
               "dl_sgd_step: Nesterov momentum needs momentum != 0 and dampening == 0");
  return sgd_launch("dl_sgd_step", p, g, momentum != 0.0f ? buf : nullptr, n, lr, momentum, dampening, weight_decay, grad_scale,
                    nullptr, coef, flags, stream);
}
extern "C" int dl_sgd_step_dev(float* p, const float* g, float* buf, int64_t n, const float* hyper, const float* coef, int flags,
                               dl_stream_t stream) {
  DL_CHECK_ARG(hyper, "dl_sgd_step_dev: bad args (hyper is null)");
  DL_CHECK_ARG(!(flags & DL_SGD_FIRST), "dl_sgd_step_dev: DL_SGD_FIRST is refused, the momentum buffer must already exist");
  DL_CHECK_ARG(!(flags & DL_SGD_NESTEROV) || buf, "dl_sgd_step_dev: Nesterov momentum needs a momentum buffer");
  return sgd_launch("dl_sgd_step_dev", p, g, buf, n, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, hyper, coef, flags, stream);
}

__global__ void ema_k(float* __restrict__ ema, const float* __restrict__ p, float w, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const float e = ema[i];
    ema[i] = e + w * (p[i] - e);
  }
}
extern "C" int dl_ema_update(float* ema, const float* p, float beta, int64_t n, dl_stream_t stream) {
  DL_CHECK_ARG(ema && p && n > 0, "dl_ema_update: bad args");
  hipLaunchKernelGGL(ema_k, ew_grid(n), 256, 0, (hipStream_t)stream, ema, p, 1.0f - beta, n);
  DL_LAUNCH_CHECK();
  return DL_OK;
}

__global__ void cast_f2b_k(const float* __restrict__ s, bf16_t* __restrict__ d, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) d[i] = f2bf(s[i]);
}
__global__ void cast_b2f_k(const bf16_t* __restrict__ s, float* __restrict__ d, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) d[i] = bf2f(s[i]);
}
extern "C" int dl_cast_f32_to_bf16(const float* src, void* dst, int64_t n, dl_stream_t stream) {
  DL_CHECK_ARG(src && dst && n > 0, "dl_cast_f32_to_bf16: bad args");
  hipLaunchKernelGGL(cast_f2b_k, ew_grid(n), 256, 0, (hipStream_t)stream, src, (bf16_t*)dst, n);
  DL_LAUNCH_CHECK();
  return DL_OK;
}
// strided rows: dst[r, c] = bf16(src[r, c]) for r < rows, c < cols (cols % 4 == 0; both row strides in elements)
__global__ void cast2d_f2b_k(const float* __restrict__ s, int64_t lds, bf16_t* __restrict__ d, int64_t ldd, int64_t rows, int cols4) {
  const int64_t n = rows * cols4;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / cols4;
    const int c = (int)(i - r * cols4) * 4;
    const f32x4_t v = *(const f32x4_t*)(s + r * lds + c);
    uint2 o;
    o.x = pack2bf(v[0], v[1]);
    o.y = pack2bf(v[2], v[3]);
    *(uint2*)(d + r * ldd + c) = o;
  }
}
extern "C" int dl_cast2d_f32_to_bf16(const float* src, int64_t ld_src, void* dst, int64_t ld_dst, int64_t rows, int64_t cols,
                                     dl_stream_t stream) {
  DL_CHECK_ARG(src && dst && rows > 0 && cols > 0 && cols % 4 == 0 && ld_src % 4 == 0 && ld_dst % 4 == 0 &&
                   (((uintptr_t)src & 15) | ((uintptr_t)dst & 7)) == 0,
               "dl_cast2d_f32_to_bf16: cols, strides %% 4 and 16 / 8-byte alignment");
  hipLaunchKernelGGL(cast2d_f2b_k, ew_grid(rows * cols / 4), 256, 0, (hipStream_t)stream, src, ld_src, (bf16_t*)dst, ld_dst, rows,
                     (int)(cols / 4));
  DL_LAUNCH_CHECK();
  return DL_OK;
}
extern "C" int dl_cast_bf16_to_f32(const void* src, float* dst, int64_t n, dl_stream_t stream) {
  DL_CHECK_ARG(src && dst && n > 0, "dl_cast_bf16_to_f32: bad args");
  hipLaunchKernelGGL(cast_b2f_k, ew_grid(n), 256, 0, (hipStream_t)stream, (const bf16_t*)src, dst, n);
  DL_LAUNCH_CHECK();
  return DL_OK;
}

// f32 [R,C] -> bf16 dst [R, ld_dst] and/or transposed dstT [C, ld_t]; 32x32 tiles through LDS so both the
// read and the two writes are coalesced.  Padding columns are zero-filled.
__global__ void cast_weight_k(const float* __restrict__ src, int64_t R, int64_t C, bf16_t* __restrict__ dst,
                              int64_t ld_dst, bf16_t* __restrict__ dstT, int64_t ld_t) {
  __shared__ float tile[32][33];
  const int64_t r0 = (int64_t)blockIdx.y * 32, c0 = (int64_t)blockIdx.x * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 256 threads: ty 0..7
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int64_t r = r0 + ty + j * 8, c = c0 + tx;
    const float v = (r < R && c < C) ? src[r * C + c] : 0.0f;
    tile[ty + j * 8][tx] = v;
    if (dst && r < R && c < ld_dst) dst[r * ld_dst + c] = f2bf(v);
  }
  __syncthreads();
  if (dstT) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t c = c0 + ty + j * 8, r = r0 + tx;  // dstT[c][r]
      if (c < C && r < ld_t) dstT[c * ld_t + r] = f2bf(tile[tx][ty + j * 8]);
    }
  }
}
extern "C" int dl_cast_weight(const float* src, int64_t R, int64_t C, void* dst, int64_t ld_dst, void* dstT,
                              int64_t ld_t, dl_stream_t stream) {
  DL_CHECK_ARG(src && R > 0 && C > 0 && (dst || dstT), "dl_cast_weight: bad args");
  DL_CHECK_ARG(!dst || ld_dst >= C, "dl_cast_weight: ld_dst < C");
  DL_CHECK_ARG(!dstT || ld_t >= R, "dl_cast_weight: ld_t < R");
  const int64_t cmax = dst ? (ld_dst > C ? ld_dst : C) : C;
  const int64_t rmax = dstT ? (ld_t > R ? ld_t : R) : R;
  dim3 grid(cdiv(cmax, 32), cdiv(rmax, 32));
  hipLaunchKernelGGL(cast_weight_k, grid, 256, 0, (hipStream_t)stream, src, R, C, (bf16_t*)dst, ld_dst, (bf16_t*)dstT,
                     ld_t);
  DL_LAUNCH_CHECK();
  return DL_OK;
}

// every bf16 weight shadow of a network in ONE launch: a device table of descriptors, one 32x32 tile per workgroup
__global__ void cast_weights_batched_k(const dl_cast_desc_t* __restrict__ desc, int n_desc) {
  __shared__ float tile[32][33];
  int lo = 0, hi = n_desc - 1;  // last descriptor whose tile_begin <= blockIdx.x
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (desc[mid].tile_begin <= (int64_t)blockIdx.x) lo = mid;
    else hi = mid - 1;
  }
  const dl_cast_desc_t d = desc[lo];
  const int64_t t = (int64_t)blockIdx.x - d.tile_begin;
  const int64_t r0 = (t / d.tiles_c) * 32, c0 = (t % d.tiles_c) * 32;
  const float* src = (const float*)d.src;
  bf16_t* dst = (bf16_t*)d.dst;
  bf16_t* dstT = (bf16_t*)d.dst_t;
  bf16_t* dstP = (bf16_t*)d.dst_swiglu;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int64_t r = r0 + ty + j * 8, c = c0 + tx;
    const float v = (r < d.R && c < d.C) ? src[r * d.C + c] : 0.0f;
    tile[ty + j * 8][tx] = v;
    if (dst && r < d.R && c < d.ld_dst) dst[r * d.ld_dst + c] = f2bf(v);
    if (dstP && r < d.R && c < d.ld_swiglu) {  // row order of dl_cast_weight_swiglu: 32-row groups [16 x1 | 16 x3]
      const int64_t F = d.R >> 1;
      const int64_t rr = r < F ? r : r - F;
      dstP[((rr >> 4) * 32 + (r < F ? 0 : 16) + (rr & 15)) * d.ld_swiglu + c] = f2bf(v);
    }
  }
  __syncthreads();
  if (dstT) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t c = c0 + ty + j * 8, r = r0 + tx;
      if (c < d.C && r < d.ld_t) dstT[c * d.ld_t + r] = f2bf(tile[tx][ty + j * 8]);
    }
  }
}
extern "C" int dl_cast_weights_batched(const dl_cast_desc_t* desc_dev, int n_desc, int64_t total_tiles, dl_stream_t stream) {
  DL_CHECK_ARG(desc_dev && n_desc > 0 && total_tiles > 0 && total_tiles < (1ll << 31), "dl_cast_weights_batched: bad args");
  hipLaunchKernelGGL(cast_weights_batched_k, (int)total_tiles, 256, 0, (hipStream_t)stream, desc_dev, n_desc);
  DL_LAUNCH_CHECK();
  return DL_OK;
}

// row-permuted bf16 copy of the packed SwiGLU weight (see dl_gemm_nt_swiglu): dst row n' <- src row perm(n')
__global__ void cast_weight_swiglu_k(const float* __restrict__ src, int F, int C, bf16_t* __restrict__ dst, int64_t ld) {
  const int64_t total = (int64_t)2 * F * ld, stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int c = (int)(i % ld);
    const int np = (int)(i / ld);
    const int q = np >> 5, s = np & 31;  // 32-row groups: 16 x1 rows then the 16 x3 rows of the same hidden units
    const int srow = (s < 16) ? (16 * q + s) : (F + 16 * q + (s - 16));
    dst[i] = c < C ? f2bf(src[(int64_t)srow * C + c]) : (bf16_t)0;
  }
}
extern "C" int dl_cast_weight_swiglu(const float* src, int64_t F, int64_t C, void* dst, int64_t ld_dst, dl_stream_t stream) {
  DL_CHECK_ARG(src && dst && F > 0 && F % 16 == 0 && C > 0 && ld_dst >= C, "dl_cast_weight_swiglu: bad args");
  hipLaunchKernelGGL(cast_weight_swiglu_k, ew_grid(2 * F * ld_dst), 256, 0, (hipStream_t)stream, src, (int)F, (int)C,
                     (bf16_t*)dst, ld_dst);
  DL_LAUNCH_CHECK();
  return DL_OK;
}
