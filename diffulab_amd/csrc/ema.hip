// Post-hoc EMA (Karras et al. 2024, "Analyzing and Improving the Training Dynamics of Diffusion Models", sec. 3.2 / app. C) over the
// flat f32 parameter arenas: the profile update of up to four EMA copies in one pass over the online parameters, and the synthesis
// of an EMA of any length as a weighted sum of stored snapshots.  Both are streaming kernels: float4 per lane, ew_grid's capped
// grid with a grid-stride loop, a scalar tail for n % 4; no atomics, the same bits on every run.
#include <math.h>

#include "common.h"

#define EMA_MAX_PROFILES 4
#define LINCOMB_MAX_SOURCES 256
#define LINCOMB_UNROLL 8  // sources whose loads are in flight before the first multiply-add of the group

// ---------------------------------------------------------------- profile update
struct EmaProfiles {
  float* ema[EMA_MAX_PROFILES];
  float w[EMA_MAX_PROFILES];
};

// One element.  The middle expression is ema_k's (elementwise.hip), under the same contraction setting (the compiler's default:
// one fused multiply-add of w, p - e and e), so with K = 1 and 0 < w < 1 the bits are dl_ema_update's.  w == 1 and w == 0 are exact:
// e + 1 * (p - e) rounds twice and is p only where p - e is exact, and e + 0 * (p - e) turns -0 into +0 and a non-finite p - e into NaN.
__device__ __forceinline__ float ema_elem(float e, float p, float w) {
  const float r = e + w * (p - e);
  return w == 1.0f ? p : (w == 0.0f ? e : r);
}

template <int K>
__global__ __launch_bounds__(256) void ema_multi_k(EmaProfiles a, const float* __restrict__ p, int64_t n4, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t gi = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (int64_t i = gi; i < n4; i += stride) {
    const f32x4_t pp = ((const f32x4_t*)p)[i];
    f32x4_t e[K];
#pragma unroll
    for (int k = 0; k < K; ++k) e[k] = ((const f32x4_t*)a.ema[k])[i];
#pragma unroll
    for (int k = 0; k < K; ++k) {
#pragma unroll
      for (int j = 0; j < 4; ++j) e[k][j] = ema_elem(e[k][j], pp[j], a.w[k]);
      ((f32x4_t*)a.ema[k])[i] = e[k];
    }
  }
  // tail (n - 4 n4 elements: n % 4, or all of n where a pointer is off the 16-byte grid and n4 == 0)
  for (int64_t i = n4 * 4 + gi; i < n; i += stride) {
    const float pj = p[i];
#pragma unroll
    for (int k = 0; k < K; ++k) a.ema[k][i] = ema_elem(a.ema[k][i], pj, a.w[k]);
  }
}

extern "C" int dl_ema_update_multi(float* ema0, float* ema1, float* ema2, float* ema3, const float* p, int K, float w0, float w1,
                                   float w2, float w3, int64_t n, dl_stream_t stream) {
  DL_CHECK_ARG(K >= 1 && K <= EMA_MAX_PROFILES, "dl_ema_update_multi: K %d (1 .. %d profiles)", K, EMA_MAX_PROFILES);
  EmaProfiles a = {{ema0, ema1, ema2, ema3}, {w0, w1, w2, w3}};
  DL_CHECK_ARG(p && n > 0, "dl_ema_update_multi: null p or n %lld <= 0", (long long)n);
  uintptr_t bits = (uintptr_t)p;
  for (int k = 0; k < K; ++k) {
    DL_CHECK_ARG(a.ema[k], "dl_ema_update_multi: profile %d of %d is NULL", k, K);
    DL_CHECK_ARG(isfinite(a.w[k]), "dl_ema_update_multi: weight %d is not finite", k);
    DL_CHECK_ARG(a.ema[k] != p, "dl_ema_update_multi: profile %d is the parameter buffer itself", k);
    for (int j = 0; j < k; ++j) DL_CHECK_ARG(a.ema[j] != a.ema[k], "dl_ema_update_multi: profiles %d and %d are one buffer", j, k);
    bits |= (uintptr_t)a.ema[k];
  }
  DL_CHECK_ARG((bits & 3) == 0, "dl_ema_update_multi: 4B alignment");
  const int64_t n4 = (bits & 15) == 0 ? n / 4 : 0;  // float4 only where every pointer allows it
  const int64_t n_scalar = n - 4 * n4;
  const int grid = ew_grid(n4 > n_scalar ? n4 : n_scalar);
#define EMA_LAUNCH(KK) hipLaunchKernelGGL(ema_multi_k<KK>, grid, 256, 0, (hipStream_t)stream, a, p, n4, n)
  switch (K) {
    case 1: EMA_LAUNCH(1); break;
    case 2: EMA_LAUNCH(2); break;
    case 3: EMA_LAUNCH(3); break;
    default: EMA_LAUNCH(4); break;
  }
#undef EMA_LAUNCH
  DL_LAUNCH_CHECK();
  return DL_OK;
}

// ---------------------------------------------------------------- synthesis
// out[i] = sum_k w[k] src_k[i]: one chain acc = fma(w[k], src_k[i], acc), k = 0 .. K - 1, from 0 or (ACC) from out[i].  The tables are
// wave-uniform (scalar loads); groups of LINCOMB_UNROLL sources are loaded before their multiply-adds, so a lane keeps
// LINCOMB_UNROLL 16-byte loads in flight.
template <bool ACC>
__global__ __launch_bounds__(256) void lincomb_k(float* __restrict__ out, const int64_t* __restrict__ srcs, const float* __restrict__ w,
                                                 int K, int64_t n4, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t gi = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (int64_t i = gi; i < n4; i += stride) {
    f32x4_t acc = {0.0f, 0.0f, 0.0f, 0.0f};
    if (ACC) acc = ((const f32x4_t*)out)[i];
    int k = 0;
    for (; k + LINCOMB_UNROLL <= K; k += LINCOMB_UNROLL) {
      f32x4_t v[LINCOMB_UNROLL];
#pragma unroll
      for (int u = 0; u < LINCOMB_UNROLL; ++u) v[u] = ((const f32x4_t*)(uintptr_t)srcs[k + u])[i];
#pragma unroll
      for (int u = 0; u < LINCOMB_UNROLL; ++u) {
        const float wk = w[k + u];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = __builtin_fmaf(wk, v[u][j], acc[j]);
      }
    }
    for (; k < K; ++k) {
      const f32x4_t v = ((const f32x4_t*)(uintptr_t)srcs[k])[i];
      const float wk = w[k];
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = __builtin_fmaf(wk, v[j], acc[j]);
    }
    ((f32x4_t*)out)[i] = acc;
  }
  for (int64_t i = n4 * 4 + gi; i < n; i += stride) {  // tail (n % 4)
    float acc = ACC ? out[i] : 0.0f;
    for (int k = 0; k < K; ++k) acc = __builtin_fmaf(w[k], ((const float*)(uintptr_t)srcs[k])[i], acc);
    out[i] = acc;
  }
}

extern "C" int dl_arena_lincomb(float* out, const int64_t* srcs_host, const int64_t* srcs_dev, const float* w_host, const float* w_dev,
                                int K, int64_t n, int flags, dl_stream_t stream) {
  DL_CHECK_ARG(K >= 1 && K <= LINCOMB_MAX_SOURCES, "dl_arena_lincomb: K %d (1 .. %d sources)", K, LINCOMB_MAX_SOURCES);
  DL_CHECK_ARG(out && srcs_host && srcs_dev && w_host && w_dev, "dl_arena_lincomb: null out or table");
  DL_CHECK_ARG(n > 0, "dl_arena_lincomb: n %lld <= 0", (long long)n);
  DL_CHECK_ARG((flags & ~DL_LINCOMB_ACCUMULATE) == 0, "dl_arena_lincomb: unknown flag bits 0x%x", flags);
  DL_CHECK_ARG(((uintptr_t)out & 15) == 0 && ((uintptr_t)srcs_dev & 7) == 0 && ((uintptr_t)w_dev & 3) == 0,
               "dl_arena_lincomb: out must be 16-byte aligned, the device tables 8- and 4-byte aligned");
  for (int k = 0; k < K; ++k) {
    const uintptr_t s = (uintptr_t)srcs_host[k];
    DL_CHECK_ARG(s != 0 && (s & 15) == 0, "dl_arena_lincomb: source %d is NULL or not 16-byte aligned", k);
    DL_CHECK_ARG(s != (uintptr_t)out, "dl_arena_lincomb: out is source %d", k);
  }
  const int64_t n4 = n / 4;
  const int grid = ew_grid(n4 > 0 ? n4 : n);
  if (flags & DL_LINCOMB_ACCUMULATE)
    hipLaunchKernelGGL(lincomb_k<true>, grid, 256, 0, (hipStream_t)stream, out, srcs_dev, w_dev, K, n4, n);
  else
    hipLaunchKernelGGL(lincomb_k<false>, grid, 256, 0, (hipStream_t)stream, out, srcs_dev, w_dev, K, n4, n);
  DL_LAUNCH_CHECK();
  return DL_OK;
}
