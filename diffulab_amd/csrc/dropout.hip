// Dropout of the UNet (unet.py:171 ResBlock.out_layers, unet.py:272 AttentionBlock.to_out): a counter-based mask applied by one
// stand-alone elementwise kernel, out = fma(x, keep ? scale : 0, resid), between the launches of the block sequences.
//
// The mask is a pure function of (seed, step, site, element index): element i of the logical [rows, cols] view (pad columns of a
// pitched buffer are not counted) belongs to group g = i >> 3; Philox4x32-10 on the counter (g lo, g hi, site, step lo) under the
// key (seed lo, seed hi) gives four words = eight 16-bit halves, one per element of the group (lane i & 7: word lane >> 1, low
// half for even lanes); an element is dropped iff its half is below T = round(p * 65536).  One Philox call per 16-byte bf16
// vector; forward and backward of a site regenerate the same mask, nothing is stored.
//
// (seed, step) are read from DEVICE memory: a recorded launch plan or a captured graph that replays this launch sees the step
// the host wrote last.
#include <math.h>

#include "common.h"

#define DROP_THREADS 256
#define PHILOX_M0 0xD2511F53u
#define PHILOX_M1 0xCD9E8D57u
#define PHILOX_W0 0x9E3779B9u
#define PHILOX_W1 0xBB67AE85u

__device__ __forceinline__ u32x4_t philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(PHILOX_M0, c0), lo0 = PHILOX_M0 * c0;
    const uint32_t hi1 = __umulhi(PHILOX_M1, c2), lo1 = PHILOX_M1 * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += PHILOX_W0;
    k1 += PHILOX_W1;
  }
  u32x4_t w = {c0, c1, c2, c3};
  return w;
}

// per-element multipliers of group g: scale where the element is kept, 0 where it is dropped
__device__ __forceinline__ void drop_factors(int64_t g, uint32_t site, uint64_t seed, uint64_t step, uint32_t T, float scale,
                                             float (&m)[8]) {
  const u32x4_t w = philox4x32_10((uint32_t)g, (uint32_t)((uint64_t)g >> 32), site, (uint32_t)step, (uint32_t)seed,
                                  (uint32_t)(seed >> 32));
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    m[2 * j] = (w[j] & 0xffffu) < T ? 0.0f : scale;
    m[2 * j + 1] = (w[j] >> 16) < T ? 0.0f : scale;
  }
}

template <bool F32>
__device__ __forceinline__ void drop_load8(const void* base, int64_t off, float (&f)[8]) {
  if (F32) {
    const f32x4_t a = *(const f32x4_t*)((const float*)base + off);
    const f32x4_t b = *(const f32x4_t*)((const float*)base + off + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) f[j] = a[j], f[4 + j] = b[j];
  } else {
    unpack8(*(const u32x4_t*)((const bf16_t*)base + off), f);
  }
}
template <bool F32>
__device__ __forceinline__ void drop_store8(void* base, int64_t off, const float (&f)[8]) {
  if (F32) {
    f32x4_t a, b;
#pragma unroll
    for (int j = 0; j < 4; ++j) a[j] = f[j], b[j] = f[4 + j];
    *(f32x4_t*)((float*)base + off) = a;
    *(f32x4_t*)((float*)base + off + 4) = b;
  } else {
    *(u32x4_t*)((bf16_t*)base + off) = pack8(f);
  }
}

// One thread per group of 8 elements and iteration, grid-stride over the ngroups = rows * cols / 8 groups.  `out` may alias `x`
// (and `resid`): a thread reads its group of every operand before it writes it, and no other thread touches that group.
// DENSE: every pitch equals cols, so the element offset is 8 g; otherwise (row, column group) = divmod(g, cols / 8).
template <bool F32, bool DENSE>
__global__ __launch_bounds__(DROP_THREADS) void dropout_k(const void* x, int64_t ldx, const void* resid, int64_t ldr, void* out,
                                                          int64_t ldo, int64_t ngroups, int64_t cpg,
                                                          const uint64_t* __restrict__ rng_state, uint32_t site, uint32_t T,
                                                          float scale) {
  const uint64_t seed = rng_state[0], step = rng_state[1];
  const int64_t stride = (int64_t)gridDim.x * DROP_THREADS;
  for (int64_t g = (int64_t)blockIdx.x * DROP_THREADS + threadIdx.x; g < ngroups; g += stride) {
    int64_t ox, orr, oo;
    if (DENSE) {
      ox = orr = oo = g * 8;
    } else {
      int64_t row, cg;
      if (((uint64_t)g >> 32) == 0 && ((uint64_t)cpg >> 32) == 0) {  // (a 64-bit division is ~10x the 32-bit one)
        row = (uint32_t)g / (uint32_t)cpg;
        cg = (uint32_t)g - (uint32_t)row * (uint32_t)cpg;
      } else {
        row = g / cpg;
        cg = g - row * cpg;
      }
      ox = row * ldx + cg * 8, orr = row * ldr + cg * 8, oo = row * ldo + cg * 8;
    }
    float m[8], v[8], r[8];
    drop_factors(g, site, seed, step, T, scale, m);
    drop_load8<F32>(x, ox, v);
    if (resid) {
      drop_load8<F32>(resid, orr, r);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) r[j] = 0.0f;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = __builtin_fmaf(v[j], m[j], r[j]);
    drop_store8<F32>(out, oo, v);
  }
}

extern "C" int dl_dropout(const void* x, int64_t ldx, const void* resid, int64_t ldr, void* out, int64_t ldo, int64_t rows,
                          int64_t cols, int dtype, const uint64_t* rng_state, int32_t site, int32_t T, float scale,
                          dl_stream_t stream) {
  DL_CHECK_ARG(x && out && rng_state, "dl_dropout: null x / out / rng_state");
  DL_CHECK_ARG(dtype == DL_BF16 || dtype == DL_F32, "dl_dropout: dtype %d (DL_BF16 or DL_F32)", dtype);
  const int64_t lim = (int64_t)1 << 40;
  DL_CHECK_ARG(rows > 0 && cols > 0 && rows < lim && cols < lim && rows * cols < lim,
               "dl_dropout: rows %lld x cols %lld (both positive, rows * cols < 2^40)", (long long)rows, (long long)cols);
  DL_CHECK_ARG(cols % 8 == 0, "dl_dropout: cols %lld is not a multiple of 8", (long long)cols);
  if (!resid) ldr = cols;  // (not read)
  DL_CHECK_ARG(ldx % 8 == 0 && ldr % 8 == 0 && ldo % 8 == 0 && ldx >= cols && ldr >= cols && ldo >= cols && ldx < lim && ldr < lim &&
                   ldo < lim,
               "dl_dropout: pitches %lld / %lld / %lld (multiples of 8, >= cols %lld)", (long long)ldx, (long long)ldr, (long long)ldo,
               (long long)cols);
  DL_CHECK_ARG((((uintptr_t)x | (uintptr_t)resid | (uintptr_t)out) & 15) == 0 && ((uintptr_t)rng_state & 7) == 0,
               "dl_dropout: x / resid / out must be 16-byte aligned, rng_state 8-byte aligned");
  DL_CHECK_ARG(T >= 0 && T < 65536, "dl_dropout: threshold T %d (0 <= T < 65536 = p quantised to 1 / 65536)", (int)T);
  DL_CHECK_ARG(site >= 0, "dl_dropout: site %d", (int)site);
  DL_CHECK_ARG(isfinite(scale), "dl_dropout: scale is not finite");
  const int64_t cpg = cols / 8, ngroups = rows * cpg;
  const bool dense = ldx == cols && ldr == cols && ldo == cols;
  const int grid = ew_grid(ngroups, DROP_THREADS);
#define DROP_LAUNCH(F32, DENSE)                                                                                                    \
  hipLaunchKernelGGL((dropout_k<F32, DENSE>), grid, DROP_THREADS, 0, (hipStream_t)stream, x, ldx, resid, ldr, out, ldo, ngroups, \
                     cpg, rng_state, (uint32_t)site, (uint32_t)T, scale)
  if (dtype == DL_F32) {
    if (dense) DROP_LAUNCH(true, true); else DROP_LAUNCH(true, false);
  } else {
    if (dense) DROP_LAUNCH(false, true); else DROP_LAUNCH(false, false);
  }
#undef DROP_LAUNCH
  DL_LAUNCH_CHECK();
  return DL_OK;
}
