// Gradient clipping by global norm over the flat f32 gradient arena: a fixed-order sum of squares (no atomics: the training step
// stays bit-reproducible), a one-workgroup f64 fold that leaves {total_norm, coef} in device memory, and the in-place scale for
// optimizers other than the fused AdamW (which takes the coefficient pointer itself: elementwise.hip, dl_adamw_step_clip).
#include <math.h>

#include "common.h"

// ---------------------------------------------------------------- sum of squares
// One pass, HBM-bound: 256 threads x SS_U float4 loads per thread and iteration = 16 KiB per workgroup in flight, at most SS_GRID
// workgroups (two per CU: the ~32 KiB per CU a streaming read wants), grid-stride beyond that.  Every loaded element has its own
// accumulator per thread (SS_U x 4 = 16 independent f32 chains), so a chain grows by ONE term per iteration.
#define SS_THREADS 256
#define SS_U 4
#define SS_TILE_VEC (SS_THREADS * SS_U)  // float4 per workgroup and iteration
#define SS_GRID 512
// additions after the per-thread loop: 4 levels over the 16 accumulators, 6 levels inside the wave (wave_sum), 2 over the 4 waves
#define SS_TREE_TERMS 12

static inline int64_t ss_tiles(int64_t n) {
  const int64_t nvec = n / 4;  // (an unaligned start only lowers the vector count)
  return (nvec + SS_TILE_VEC - 1) / SS_TILE_VEC;
}
static inline int64_t ss_grid(int64_t n) {
  const int64_t t = ss_tiles(n);
  return t < 1 ? 1 : (t > SS_GRID ? SS_GRID : t);
}
extern "C" int64_t dl_grad_sumsq_slots(int64_t n) { return n > 0 ? ss_grid(n) : 0; }
extern "C" int64_t dl_grad_sumsq_chain(int64_t n) {
  if (n <= 0) return 0;
  const int64_t g = ss_grid(n);
  const int64_t iters = (ss_tiles(n) + g - 1) / g;
  return iters + 1 + SS_TREE_TERMS;  // + 1: the head / tail element a thread of workgroup 0 may add
}

__global__ __launch_bounds__(SS_THREADS) void grad_sumsq_k(const float* __restrict__ x, int64_t n, int64_t head, int64_t nvec,
                                                            float* __restrict__ partials) {
  __shared__ float wsum[SS_THREADS / DL_WAVE];
  const float4* __restrict__ xv = (const float4*)(x + head);  // 16-byte aligned by construction of `head`
  float4 acc[SS_U];
#pragma unroll
  for (int u = 0; u < SS_U; ++u) acc[u] = make_float4(0.f, 0.f, 0.f, 0.f);
  const int64_t stride = (int64_t)gridDim.x * SS_TILE_VEC;
  for (int64_t base = (int64_t)blockIdx.x * SS_TILE_VEC; base < nvec; base += stride) {
    float4 v[SS_U];
#pragma unroll
    for (int u = 0; u < SS_U; ++u) {
      const int64_t i = base + (int64_t)u * SS_THREADS + threadIdx.x;
      v[u] = i < nvec ? xv[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int u = 0; u < SS_U; ++u) {
      acc[u].x = fmaf(v[u].x, v[u].x, acc[u].x);
      acc[u].y = fmaf(v[u].y, v[u].y, acc[u].y);
      acc[u].z = fmaf(v[u].z, v[u].z, acc[u].z);
      acc[u].w = fmaf(v[u].w, v[u].w, acc[u].w);
    }
  }
  // scalar head (before the first 16-byte boundary) and tail (n - head not a multiple of 4): at most 3 + 3 elements, one each for
  // the first threads of workgroup 0
  if (blockIdx.x == 0) {
    const int64_t tail0 = head + nvec * 4;
    const int64_t t = threadIdx.x;
    if (t < head) {
      acc[0].x = fmaf(x[t], x[t], acc[0].x);
    } else if (t - head < n - tail0) {
      const float e = x[tail0 + (t - head)];
      acc[0].x = fmaf(e, e, acc[0].x);
    }
  }
  float s[SS_U];
#pragma unroll
  for (int u = 0; u < SS_U; ++u) s[u] = (acc[u].x + acc[u].y) + (acc[u].z + acc[u].w);
  const float ws = wave_sum((s[0] + s[1]) + (s[2] + s[3]));
  if ((threadIdx.x & (DL_WAVE - 1)) == 0) wsum[threadIdx.x / DL_WAVE] = ws;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

extern "C" int dl_grad_sumsq(const float* x, int64_t n, float* partials, int64_t slot, int64_t capacity, dl_stream_t stream) {
  if (!(x && partials && n > 0 && slot >= 0) || (((uintptr_t)x | (uintptr_t)partials) & 3)) {
    dl_set_error("dl_grad_sumsq: bad args");
    return DL_ERR_INVALID;
  }
  const int64_t g = ss_grid(n);
  if (slot + g > capacity) {
    dl_set_error("dl_grad_sumsq: %lld slots from %lld do not fit the %lld of the partials buffer", (long long)g, (long long)slot,
                 (long long)capacity);
    return DL_ERR_INVALID;
  }
  int64_t head = (int64_t)(((16 - ((uintptr_t)x & 15)) & 15) / 4);
  if (head > n) head = n;
  const int64_t nvec = (n - head) / 4;
  hipLaunchKernelGGL(grad_sumsq_k, (int)g, SS_THREADS, 0, (hipStream_t)stream, x, n, head, nvec, partials + slot);
  DL_LAUNCH_CHECK();
  return (int)g;
}

// ---------------------------------------------------------------- fold + coefficient
// One workgroup: thread t sums its contiguous run of slots serially in f64, the 256 runs are combined by an adjacent-pair tree (slot
// order is kept, the association is fixed).  torch.nn.utils.clip_grad_norm_'s rule: coef = clamp(max_norm / (norm + 1e-6), max=1) in
// f32 on the f32 norm; an infinite norm gives 0 and a NaN norm NaN (the comparison below is false for NaN), neither is special-cased.
#define CC_THREADS 256
__global__ __launch_bounds__(CC_THREADS) void clip_coef_k(const float* __restrict__ partials, int64_t n_slots, float grad_scale,
                                                           const float* __restrict__ hyper, float max_norm,
                                                           float* __restrict__ out) {
  __shared__ double red[CC_THREADS];
  const int64_t per = (n_slots + CC_THREADS - 1) / CC_THREADS;
  const int64_t lo = (int64_t)threadIdx.x * per;
  const int64_t hi = lo + per < n_slots ? lo + per : n_slots;
  double s = 0.0;
  for (int64_t i = lo; i < hi; ++i) s += (double)partials[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = 1; w < CC_THREADS; w <<= 1) {
    if ((threadIdx.x & (2 * w - 1)) == 0) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float gs = hyper ? hyper[7] : grad_scale;
    const float norm = (float)((double)gs * sqrt(red[0]));
    const float c = max_norm / (norm + 1e-6f);
    out[0] = norm;
    out[1] = c > 1.0f ? 1.0f : c;
  }
}
extern "C" int dl_clip_coef(const float* partials, int64_t n_slots, float grad_scale, const float* hyper, float max_norm, float* out,
                            dl_stream_t stream) {
  DL_CHECK_ARG(partials && out && n_slots > 0, "dl_clip_coef: bad args");
  hipLaunchKernelGGL(clip_coef_k, 1, CC_THREADS, 0, (hipStream_t)stream, partials, n_slots, grad_scale, hyper, max_norm, out);
  DL_LAUNCH_CHECK();
  return DL_OK;
}

// ---------------------------------------------------------------- g *= *coef (optimizers that do not take the coefficient themselves)
__global__ void scale_inplace_k(float* __restrict__ g, int64_t n, int64_t head, int64_t nvec, const float* __restrict__ coef) {
  const float c = *coef;
  if (c == 1.0f) return;  // nothing was clipped: leave the buffer alone (x * 1 is x, the pass would only move bytes)
  float4* __restrict__ gv = (float4*)(g + head);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t gi = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (int64_t i = gi; i < nvec; i += stride) {
    float4 v = gv[i];
    v.x *= c, v.y *= c, v.z *= c, v.w *= c;
    gv[i] = v;
  }
  const int64_t tail0 = head + nvec * 4;
  if (gi < head) {
    g[gi] *= c;
  } else if (gi - head < n - tail0) {
    g[tail0 + (gi - head)] *= c;
  }
}
extern "C" int dl_scale_inplace(float* g, int64_t n, const float* coef, dl_stream_t stream) {
  DL_CHECK_ARG(g && coef && n > 0 && ((uintptr_t)g & 3) == 0, "dl_scale_inplace: bad args");
  int64_t head = (int64_t)(((16 - ((uintptr_t)g & 15)) & 15) / 4);
  if (head > n) head = n;
  const int64_t nvec = (n - head) / 4;
  int64_t grid = (nvec + 255) / 256;
  grid = grid < 1 ? 1 : (grid > 2048 ? 2048 : grid);  // 256 CUs x 8 workgroups, grid-stride beyond that
  hipLaunchKernelGGL(scale_inplace_k, (int)grid, 256, 0, (hipStream_t)stream, g, n, head, nvec, coef);
  DL_LAUNCH_CHECK();
  return DL_OK;
}
