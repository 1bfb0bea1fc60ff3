// HBM-bound kernels of the loss heads: MSE, the hybrid and gd heads, the variational bound per row, the flow NLL, the row head, the
// loss history and the timestep draw.  Reductions are two-stage with a fixed order: no floating-point atomics.
#include "common.h"
#include "gaussian.h"

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

// ---------------------------------------------------------------- hybrid loss of a learned-variance model
// L_simple + L_vlb of Nichol & Dhariwal, "Improved Denoising Diffusion Probabilistic Models" (2021), eq. 16, which the reference
// announces and leaves unwritten (gaussian_diffusion.py:267).  One element's variational-bound term in nats and, where GRAD, its
// derivative with respect to the raw variance output v.  The predicted mean m_p is a constant of that term (the paper's stop-gradient):
// nothing flows into the mean output from here.  tab as the learned-variance ddpm_step_k reads it.
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
// partial[0 .. np) and partial[np .. 2 np) of gd_partial_k<true, .> (below) -> loss[0] = the MSE, loss[1] = the bound in bits per dimension
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

// ---------------------------------------------------------------- loss head of every parameterisation
// dl_mse_loss_* (mode EPS) generalised: the regression target of the mean output is formed per element from eps,
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
// mse_partial_k.  W false is w == 1: the sum is then accumulated as that kernel accumulates it (acc += d * d), so that the epsilon
// target reproduces its scalar bit for bit.  HYBRID (dl_vlb_loss_*): the mean half is regressed on the tensor passed as `eps`
// whatever `target` is, which then only tells the bound how to read the mean output (the sampler's mean_type).
template <bool LV, bool W, bool HYBRID = false>
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
      const gd_elem g = gd_load<LV, W>(i, pred, eps, x0, xt, t, tab, T, HYBRID ? DL_MEAN_EPSILON : target, chw);
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
template <bool LV, bool W, bool HYBRID = false>
__global__ void gd_bwd_k(const float* __restrict__ pred, const float* __restrict__ eps, const float* __restrict__ x0,
                         const float* __restrict__ xt, const int32_t* __restrict__ t, const float* __restrict__ tab, int32_t T,
                         int target, const float* __restrict__ weight, int var_mode, float coef_m, float coef_v,
                         const float* __restrict__ g_mse, const float* __restrict__ g_vb, float* __restrict__ dpred, int64_t n,
                         int64_t chw) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  if (g_mse) coef_m *= *g_mse;  // as mse_bwd_k forms its coefficient
  if (LV && g_vb) coef_v *= *g_vb;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const gd_elem g = gd_load<LV, W>(i, pred, eps, x0, xt, t, tab, T, HYBRID ? DL_MEAN_EPSILON : target, chw);
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

// The hybrid head of a learned-variance model (L_simple + L_vlb, eq. 16): the unweighted LV kernels above, HYBRID.
extern "C" int dl_vlb_loss_fwd(const float* pred, const float* eps, const float* x0, const float* xt, const int32_t* t,
                               const float* tables, int32_t T, int mean_type, int var_mode, float* partial, float* loss,
                               int64_t batch, int64_t chw, dl_stream_t stream) {
  DL_CHECK_ARG(pred && eps && x0 && xt && t && tables && batch > 0 && chw > 0 && T > 0, "dl_vlb_loss_fwd: bad args");
  DL_CHECK_ARG(mean_type >= 0 && mean_type <= 2, "dl_vlb_loss_fwd: mean_type %d", mean_type);
  DL_CHECK_ARG(var_mode == DL_VAR_LEARNED || var_mode == DL_VAR_LEARNED_RANGE, "dl_vlb_loss_fwd: var_mode %d", var_mode);
  DL_CHECK_ARG(partial && loss, "dl_vlb_loss_fwd: bad args (partial, loss)");
  const int64_t n = batch * chw, np = dl_mse_loss_partials(n);
  hipLaunchKernelGGL((gd_partial_k<true, false, true>), (int)np, MSE_BLOCK, 0, (hipStream_t)stream, pred, eps, x0, xt, t, tables, T,
                     mean_type, nullptr, var_mode, partial, np, n, chw);
  hipLaunchKernelGGL(vlb_final_k, 1, 256, 0, (hipStream_t)stream, partial, loss, np, (float)(1.0 / (double)n),
                     (float)(1.0 / ((double)n * 0.6931471805599453)));
  DL_LAUNCH_CHECK();
  return DL_OK;
}
extern "C" int dl_vlb_loss_bwd(const float* pred, const float* eps, const float* x0, const float* xt, const int32_t* t,
                               const float* tables, int32_t T, int mean_type, int var_mode, const float* g_mse_dev,
                               const float* g_vb_dev, float* dpred, int64_t batch, int64_t chw, dl_stream_t stream) {
  DL_CHECK_ARG(pred && eps && x0 && xt && t && tables && batch > 0 && chw > 0 && T > 0, "dl_vlb_loss_bwd: bad args");
  DL_CHECK_ARG(mean_type >= 0 && mean_type <= 2, "dl_vlb_loss_bwd: mean_type %d", mean_type);
  DL_CHECK_ARG(var_mode == DL_VAR_LEARNED || var_mode == DL_VAR_LEARNED_RANGE, "dl_vlb_loss_bwd: var_mode %d", var_mode);
  DL_CHECK_ARG(dpred, "dl_vlb_loss_bwd: bad args (dpred)");
  const int64_t n = batch * chw;
  hipLaunchKernelGGL((gd_bwd_k<true, false, true>), ew_grid(n), 256, 0, (hipStream_t)stream, pred, eps, x0, xt, t, tables, T, mean_type,
                     nullptr, var_mode, (float)(2.0 / (double)n), (float)(1.0 / ((double)n * 0.6931471805599453)), g_mse_dev, g_vb_dev,
                     dpred, n, chw);
  DL_LAUNCH_CHECK();
  return DL_OK;
}

// ---------------------------------------------------------------- variational bound per (sample, timestep): evaluation
// calc_bpd_loop of Nichol & Dhariwal (2021): what gd_partial_k<true, .> sums over the whole batch, kept per row, for fixed variances too, next
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
