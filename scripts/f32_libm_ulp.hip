// One-off measurement: the error, in f32 ulps against fp64, of the library functions the fp32-regime kernels call (csrc/f32.hip):
// expf, erff, sinf, cosf, sqrtf, the division 1.0f / x and the division x / y.  The allowances of tests/f32_bounds.py (EXP_ULP, ...)
// are twice the maxima this prints, rounded up to a whole ulp.
//
// Build with the flags of csrc/Makefile (they decide which expansion of each function the compiler emits) and run on the GPU:
//     hipcc -O3 -std=c++17 --offload-arch=gfx950 -munsafe-fp-atomics scripts/f32_libm_ulp.hip -o f32_libm_ulp && ./f32_libm_ulp
//
// Sweep: every `stride`-th f32 bit pattern with lo <= |x| <= hi, both signs where the kernels see both (default stride 3: 2.8e6
// arguments per binade).  Ranges follow what the kernels and their tests feed:
//     expf   [-104, 88]        softmax s - max (down to the underflow), silu's exp(-x), the embedding's exp(-ln(P) k / half)
//     erff   [-24, 24]         GEGLU at |g| <= 30: g / sqrt(2)
//     sinf / cosf  [0, 1000]   timestep embedding: t f with t <= 1000, f <= 1
//     sqrtf  [2^-40, 2^40]     var + eps, mean square + eps
//     1 / x  [2^-40, 2^40],  x / y with the same y and x = three fixed mantissas
// The fast __expf (one v_exp_f32 of x log2 e: dgelu_f of csrc/common.h, ddt_cond_bwd_k of csrc/tokens.hip) is swept over [-88, 0] and,
// for the bounds of tests/bf16_aux_bounds.py, over [-4, 4], [-8, 8] and [-16, 16]; beside the ulp error its ABSOLUTE error over
// [-88, 0] (results in (0, 1]) is printed in units of 2^-24: its relative error grows with |x| (the rounded product x log2 e) and
// passes the 8-ulp cap, the absolute one does not grow.
// The error of a result r against the fp64 value v is |r - v| / ulp(v), ulp(v) = 2^(floor(log2 |v|) - 23), |v| clamped below at
// 2^-126 (results under the normal range count in units of the smallest normal's ulp).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

enum Fn { FN_EXP, FN_ERF, FN_SIN, FN_COS, FN_SQRT, FN_RCP, FN_DIV, FN_FEXP, FN_FEXP4, FN_FEXP8, FN_FEXP16, FN_FEXP_ABS, FN_COUNT };
static const char* kNames[FN_COUNT] = {"expf", "erff", "sinf", "cosf", "sqrtf", "1.0f / x", "x / y", "__expf [-88, 0]", "__expf [-4, 4]",
                                       "__expf [-8, 8]", "__expf [-16, 16]", "__expf [-88, 0] abs / 2^-24"};

__device__ double ulp_err(float r, double v) {
  double a = fabs(v);
  if (a < 0x1p-126) a = 0x1p-126;
  int e;
  (void)frexp(a, &e);  // a = m 2^e, m in [0.5, 1)
  return fabs((double)r - v) / ldexp(1.0, e - 24);
}

// thread i of the launch takes patterns bits0 + (i + n * total) * stride; per-thread maximum into worst[i], its argument into arg[i]
__global__ void sweep_k(int fn, uint32_t bits0, uint32_t bits1, uint32_t stride, int negate, double* worst, float* arg) {
  const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x, total = gridDim.x * blockDim.x;
  double w = 0.0;
  float wa = 0.f;
  for (uint64_t b = (uint64_t)bits0 + (uint64_t)tid * stride; b <= bits1; b += (uint64_t)total * stride) {
    float x = __uint_as_float((uint32_t)b);
    if (negate) x = -x;
    double e = 0.0;
    switch (fn) {
      case FN_EXP: e = ulp_err(expf(x), exp((double)x)); break;
      case FN_ERF: e = ulp_err(erff(x), erf((double)x)); break;
      case FN_SIN: e = ulp_err(sinf(x), sin((double)x)); break;
      case FN_COS: e = ulp_err(cosf(x), cos((double)x)); break;
      case FN_SQRT: e = ulp_err(sqrtf(x), sqrt((double)x)); break;
      case FN_RCP: e = ulp_err(1.0f / x, 1.0 / (double)x); break;
      case FN_FEXP:
      case FN_FEXP4:
      case FN_FEXP8:
      case FN_FEXP16: e = ulp_err(__expf(x), exp((double)x)); break;
      case FN_FEXP_ABS: e = fabs((double)__expf(x) - exp((double)x)) * 0x1p24; break;
      case FN_DIV: {
        const float n[3] = {1.2345678f, 1.9999999f, 1.0000001f};
        for (int k = 0; k < 3; ++k) {
          const double ek = ulp_err(n[k] / x, (double)n[k] / (double)x);
          if (ek > e) e = ek;
        }
        break;
      }
    }
    if (e > w) {
      w = e;
      wa = x;
    }
  }
  worst[tid] = w;
  arg[tid] = wa;
}

static uint32_t bits_of(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
}

int main(int argc, char** argv) {
  const uint32_t stride = argc > 1 ? (uint32_t)atoi(argv[1]) : 3u;
  struct Range { int fn; float lo, hi; int negate; };
  const Range ranges[] = {
      {FN_EXP, 0x1p-30f, 88.f, 0},   {FN_EXP, 0x1p-30f, 104.f, 1}, {FN_ERF, 0x1p-30f, 24.f, 0},  {FN_ERF, 0x1p-30f, 24.f, 1},
      {FN_SIN, 0x1p-30f, 1000.f, 0}, {FN_COS, 0x1p-30f, 1000.f, 0}, {FN_SQRT, 0x1p-40f, 0x1p40f, 0},
      {FN_RCP, 0x1p-40f, 0x1p40f, 0}, {FN_DIV, 0x1p-40f, 0x1p40f, 0}, {FN_DIV, 0x1p-40f, 0x1p40f, 1},
      {FN_FEXP, 0x1p-30f, 88.f, 1}, {FN_FEXP_ABS, 0x1p-30f, 88.f, 1},
      {FN_FEXP4, 0x1p-30f, 4.f, 0}, {FN_FEXP4, 0x1p-30f, 4.f, 1}, {FN_FEXP8, 0x1p-30f, 8.f, 0}, {FN_FEXP8, 0x1p-30f, 8.f, 1},
      {FN_FEXP16, 0x1p-30f, 16.f, 0}, {FN_FEXP16, 0x1p-30f, 16.f, 1},
  };
  const int blocks = 2048, threads = 256, total = blocks * threads;
  double* d_w;
  float* d_a;
  if (hipMalloc(&d_w, total * sizeof(double)) != hipSuccess || hipMalloc(&d_a, total * sizeof(float)) != hipSuccess) {
    fprintf(stderr, "hipMalloc failed\n");
    return 1;
  }
  std::vector<double> w(total);
  std::vector<float> a(total);
  double best[FN_COUNT] = {0};
  float besta[FN_COUNT] = {0};
  uint64_t count[FN_COUNT] = {0};
  for (const Range& r : ranges) {
    const uint32_t b0 = bits_of(r.lo), b1 = bits_of(r.hi);
    hipLaunchKernelGGL(sweep_k, blocks, threads, 0, 0, r.fn, b0, b1, stride, r.negate, d_w, d_a);
    if (hipDeviceSynchronize() != hipSuccess) {
      fprintf(stderr, "sweep of %s failed: %s\n", kNames[r.fn], hipGetErrorString(hipGetLastError()));
      return 1;
    }
    (void)hipMemcpy(w.data(), d_w, total * sizeof(double), hipMemcpyDeviceToHost);
    (void)hipMemcpy(a.data(), d_a, total * sizeof(float), hipMemcpyDeviceToHost);
    count[r.fn] += ((uint64_t)b1 - b0) / stride + 1;
    for (int i = 0; i < total; ++i)
      if (w[i] > best[r.fn]) {
        best[r.fn] = w[i];
        besta[r.fn] = a[i];
      }
  }
  printf("stride %u\n", stride);
  for (int f = 0; f < FN_COUNT; ++f) {
    const int chosen = (int)ceil(2.0 * best[f] - 1e-9);
    printf("%-28s max %.4f ulp at x = %.9g (%llu arguments)  ->  allowance %d ulp%s\n", kNames[f], best[f], besta[f],
           (unsigned long long)count[f], chosen, chosen > 8 ? "  ABOVE THE 8-ULP CAP" : "");
  }
  (void)hipFree(d_w);
  (void)hipFree(d_a);
  return 0;
}
