// HBM-bound kernels: noising, optimizers, EMA, casts; the error plumbing, library info and streams of the whole library.
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
// LAB switch (not in the header): the cap a data-parallel host sets through dl_dit_block_t::max_workgroups, for the tests
extern "C" __attribute__((visibility("default"))) void dl_lab_set_wg_cap(int cap) { dl_set_wg_cap(cap); }
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

// ---------------------------------------------------------------- noising
// z = (1-t) x + t eps; chw % 4 == 0 fast path works on float4, else scalar.  One element goes through flow_noise_elem in both forms,
// with contraction off and the fused multiply-add explicit (the rounding the float4 form has always had): left to the compiler,
// the scalar form's loop was unrolled by two with the pair fused and the odd trip not, so z depended on the form and on the trip.
__device__ __forceinline__ float flow_noise_elem(const float x, const float e, const float tt) {
#pragma clang fp contract(off)
  return __builtin_fmaf(1.0f - tt, x, tt * e);
}
template <bool VEC>
__global__ void flow_add_noise_k(const float* __restrict__ x, const float* __restrict__ e,
                                 const float* __restrict__ t, float* __restrict__ z, int64_t n, int64_t chw) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  if (VEC) {
    const int64_t nv = n >> 2, cv = chw >> 2;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += stride) {
      const float tt = t[i / cv];
      const float4 a = ((const float4*)x)[i], b = ((const float4*)e)[i];
      float4 o;
      o.x = flow_noise_elem(a.x, b.x, tt);
      o.y = flow_noise_elem(a.y, b.y, tt);
      o.z = flow_noise_elem(a.z, b.z, tt);
      o.w = flow_noise_elem(a.w, b.w, tt);
      ((float4*)z)[i] = o;
    }
  } else {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) z[i] = flow_noise_elem(x[i], e[i], t[i / chw]);
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
#pragma clang fp contract(off)
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const int32_t ti = t[i / chw];
    const float ca = sqrt_ab[ti];
    const float cb = sqrtf(1.0f - ab[ti]);  // gd.py:340: sqrt evaluated in fp32 after the .float() gather
    o[i] = ca * x[i] + cb * e[i];           // (contraction off: two products and a sum on every trip of the loop)
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

// ---------------------------------------------------------------- optimizer / casts
// One element: adamw_elem (common.h), the same body in the float4 loop, in the n % 4 tail and in adamw_dev_k, so an element's result
// does not depend on where in a buffer it lies or on which entry point updates it (tests/test_step_paths_gpu.py holds that bit for bit).
// CLIP: the gradient scale is grad_scale * *coef, the clipping coefficient dl_clip_coef left in device memory (clip.hip); formed once
// per thread, so with *coef == 1 the update is bit-identical to the plain one
template <bool CLIP>
__global__ void adamw_k(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                        float* __restrict__ v, int64_t n4, int64_t n, float lr, float b1, float b2, float eps,
                        float wd, float inv_bc1_lr, float inv_sqrt_bc2, float grad_scale, const float* __restrict__ coef) {
#pragma clang fp contract(off)
  const AdamwScalars s = adamw_scalars(lr, b1, b2, eps, wd, inv_bc1_lr, inv_sqrt_bc2, CLIP ? grad_scale * *coef : grad_scale);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    float4 pp = ((float4*)p)[i], mm = ((float4*)m)[i], vv = ((float4*)v)[i];
    const float4 gg = ((const float4*)g)[i];
    adamw_elem(pp.x, gg.x, mm.x, vv.x, s);
    adamw_elem(pp.y, gg.y, mm.y, vv.y, s);
    adamw_elem(pp.z, gg.z, mm.z, vv.z, s);
    adamw_elem(pp.w, gg.w, mm.w, vv.w, s);
    ((float4*)p)[i] = pp;
    ((float4*)m)[i] = mm;
    ((float4*)v)[i] = vv;
  }
  // tail (n % 4)
  const int64_t tail0 = n4 * 4;
  const int64_t gi = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gi < n - tail0) {
    const int64_t i = tail0 + gi;
    float pj = p[i], mj = m[i], vj = v[i];
    adamw_elem(pj, g[i], mj, vj, s);
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
template <bool CLIP>
__global__ void adamw_dev_k(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                            int64_t n, const float* __restrict__ hyper, const float* __restrict__ coef) {
#pragma clang fp contract(off)
  const AdamwScalars s = adamw_scalars(hyper[0], hyper[1], hyper[2], hyper[3], hyper[4], hyper[5], hyper[6],
                                       CLIP ? hyper[7] * *coef : hyper[7]);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    float pj = p[i], mj = m[i], vj = v[i];
    adamw_elem(pj, g[i], mj, vj, s);
    p[i] = pj;
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
// fused multiply-add explicit, as in adamw_elem (common.h) and for its reason: all of them round identically, which the tests hold bit for bit.
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
