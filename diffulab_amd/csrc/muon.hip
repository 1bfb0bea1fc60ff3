// Muon (torch.optim.Muon: momentum, then quintic Newton-Schulz orthogonalisation of every hidden weight matrix in bf16) over the
// flat f32 parameter arena, with AdamW on everything that is not a Muon matrix.  The number of launches of one step does not depend
// on the number of matrices: a device table describes them all and every kernel finds its matrix through it.
//
//   dl_muon_pre            1 launch   elementwise over the arena, one workgroup per chunk of the chunk table: AdamW on auxiliary
//                                     chunks; on Muon chunks the momentum buffer, bf16(U) into the X workspace and the chunk's sum of
//                                     squares of bf16(U) (fixed order, no atomics)
//   dl_muon_orthogonalize  2 + 3 k    fold of the partial sums per matrix (f64, slot order, as dl_clip_coef folds), X = bf16(X / norm)
//                                     in place, then k times: A = X X^T, P = b A + c A A, X' = a X + P X as grouped bf16 MFMA GEMMs
//   dl_muon_post           1 launch   p = p (1 - lr wd) - lr ratio O
//
// Tall matrices (rows > cols) are NOT transposed: the iteration runs in its tall form, A = X^T X, X' = a X + X P, which is the wide
// iteration of X^T term by term.  The workspace X therefore always has the parameter's own orientation and the post pass reads O as
// the parameter is laid out.  One tile kernel serves the three phases: an operand is either contraction-contiguous (read as stored)
// or contraction-strided (transposed while it is staged into the LDS).
//
// Kernel boundaries are the only grid-wide synchronisation.
#include <math.h>

#include "common.h"

#define MU_THREADS 256
#define MU_TILE 64                    // output tile edge and the granularity of every matrix dimension
#define MU_FLAT (MU_TILE * MU_TILE)   // elements of one 64 x 64 tile: the unit of the stage and post passes
#define MU_BK 64                      // contraction step of one LDS stage
#define MU_LDS_LD (MU_BK + 8)         // LDS row pitch in bf16: 144 bytes, 16-byte aligned rows, 4-bank skew per row
#define MU_MAX_SHORT 4096
#define MU_MAX_LONG 32768
#define MU_MAX_STEPS 100              // torch refuses ns_steps >= 100

// matrix table fields (int64 each, DL_MUON_MAT_FIELDS per matrix, one sentinel row carrying the totals of SQ0 / AP0)
enum { MT_OFF = 0, MT_ROWS, MT_COLS, MT_RATIO, MT_XOFF, MT_AOFF, MT_SQ0, MT_AP0, MT_CHUNK0, MT_NCHUNK };
// chunk table fields (int64 each, DL_MUON_CHUNK_FIELDS per chunk)
enum { CK_START = 0, CK_LEN, CK_MAT };

// ---------------------------------------------------------------- host side: table validation (before any launch)
static int mu_check_mats(const char* who, const int64_t* mh, const void* md, int64_t n_mat, int64_t n_arena, int64_t x_cap,
                         int64_t a_cap) {
  DL_CHECK_ARG(n_mat >= 0 && (n_mat == 0 || (mh && md)), "%s: bad args (matrix table)", who);
  int64_t sq = 0, ap = 0, prev_end = 0;
  for (int64_t i = 0; i < n_mat; ++i) {
    const int64_t* e = mh + i * DL_MUON_MAT_FIELDS;
    const int64_t rows = e[MT_ROWS], cols = e[MT_COLS];
    DL_CHECK_ARG(rows > 0 && cols > 0, "%s: matrix %lld has shape %lld x %lld", who, (long long)i, (long long)rows, (long long)cols);
    const int64_t ms = rows < cols ? rows : cols, ml = rows < cols ? cols : rows;
    if (rows % MU_TILE || cols % MU_TILE || ms > MU_MAX_SHORT || ml > MU_MAX_LONG) {
      dl_set_error("%s: matrix %lld is %lld x %lld: both dimensions must be multiples of %d, the short one <= %d, the long one <= %d",
                   who, (long long)i, (long long)rows, (long long)cols, MU_TILE, MU_MAX_SHORT, MU_MAX_LONG);
      return DL_ERR_UNSUPPORTED;
    }
    DL_CHECK_ARG(e[MT_OFF] >= prev_end && e[MT_OFF] + rows * cols <= n_arena,
                 "%s: matrix %lld at offset %lld (%lld elements) overlaps its predecessor or leaves the buffer of %lld", who, (long long)i,
                 (long long)e[MT_OFF], (long long)(rows * cols), (long long)n_arena);
    prev_end = e[MT_OFF] + rows * cols;
    DL_CHECK_ARG(e[MT_XOFF] >= 0 && e[MT_XOFF] % 8 == 0 && e[MT_XOFF] + rows * cols <= x_cap,
                 "%s: matrix %lld does not fit the X workspace (offset %lld, capacity %lld)", who, (long long)i, (long long)e[MT_XOFF],
                 (long long)x_cap);
    DL_CHECK_ARG(e[MT_AOFF] >= 0 && e[MT_AOFF] % 8 == 0 && e[MT_AOFF] + ms * ms <= a_cap,
                 "%s: matrix %lld does not fit the A workspace (offset %lld, capacity %lld)", who, (long long)i, (long long)e[MT_AOFF],
                 (long long)a_cap);
    DL_CHECK_ARG(e[MT_SQ0] == sq && e[MT_AP0] == ap, "%s: matrix %lld has inconsistent tile prefixes", who, (long long)i);
    DL_CHECK_ARG(e[MT_CHUNK0] >= 0 && e[MT_NCHUNK] > 0, "%s: matrix %lld has no chunks", who, (long long)i);
    sq += (ms / MU_TILE) * (ms / MU_TILE);
    ap += (rows / MU_TILE) * (cols / MU_TILE);
  }
  if (n_mat > 0) {
    const int64_t* e = mh + n_mat * DL_MUON_MAT_FIELDS;
    DL_CHECK_ARG(e[MT_SQ0] == sq && e[MT_AP0] == ap && ap < (1ll << 31), "%s: the sentinel row does not carry the tile totals", who);
  }
  return DL_OK;
}

// ---------------------------------------------------------------- device helpers
__device__ __forceinline__ const int64_t* mu_row(const int64_t* __restrict__ mats, int i) { return mats + (int64_t)i * DL_MUON_MAT_FIELDS; }
// the matrix whose prefix [field] range holds tile t: the last i with mats[i][field] <= t (the sentinel row bounds the search)
__device__ __forceinline__ int mu_find(const int64_t* __restrict__ mats, int n_mat, int field, int64_t t) {
  int lo = 0, hi = n_mat - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (mu_row(mats, mid)[field] <= t) lo = mid; else hi = mid - 1;
  }
  return lo;
}
__device__ __forceinline__ float mu_block_sum(float s, float* wsum) {
  const float ws = wave_sum(s);
  if ((threadIdx.x & (DL_WAVE - 1)) == 0) wsum[threadIdx.x / DL_WAVE] = ws;
  __syncthreads();
  return (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

// ---------------------------------------------------------------- pre pass
struct MuPre {
  float lr, b1, b2, eps, wd, inv_bc1_lr, inv_sqrt_bc2;  // AdamW of the auxiliary ranges (dl_adamw_step's scalars)
  float w1, mom, gs;                                    // 1 - momentum (rounded from f64, as torch passes it to lerp_), momentum
  int nesterov;
};
// dl_adamw_step's update of one element, bit for bit: the one body every AdamW kernel of the library calls (adamw_elem, common.h)
__device__ __forceinline__ void mu_adamw_elem(float& p, const float g, float& m, float& v, const MuPre& s) {
  adamw_elem(p, g, m, v, adamw_scalars(s.lr, s.b1, s.b2, s.eps, s.wd, s.inv_bc1_lr, s.inv_sqrt_bc2, s.gs));
}
// torch's rule for one element of a Muon matrix: buf.lerp_(grad, 1 - momentum); update = grad.lerp(buf, momentum) with Nesterov,
// else buf -- lerp(start, end, w) is start + w (end - start) for w < 0.5 and end - (end - start) (1 - w) otherwise.  Returns
// bf16(update) as f32.
__device__ __forceinline__ float mu_lerp(float start, float end, float w) {
#pragma clang fp contract(off)
  const float d = end - start;
  return w < 0.5f ? start + w * d : end - d * (1.0f - w);
}
__device__ __forceinline__ float mu_muon_elem(const float g, float& b, const MuPre& s, bf16_t& ub) {
#pragma clang fp contract(off)
  const float gr = g * s.gs;
  b = mu_lerp(b, gr, s.w1);
  const float u = s.nesterov ? mu_lerp(gr, b, s.mom) : b;
  ub = f2bf(u);
  return bf2f(ub);
}

__global__ __launch_bounds__(MU_THREADS) void muon_pre_k(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                          float* __restrict__ v, const int64_t* __restrict__ chunks,
                                                          const int64_t* __restrict__ mats, bf16_t* __restrict__ xws,
                                                          float* __restrict__ partials, MuPre s, const float* __restrict__ coef) {
  __shared__ float wsum[MU_THREADS / DL_WAVE];
  if (coef) s.gs = s.gs * *coef;
  const int64_t* ck = chunks + (int64_t)blockIdx.x * DL_MUON_CHUNK_FIELDS;
  const int64_t start = ck[CK_START];
  const int len = (int)ck[CK_LEN];
  const int mat = (int)ck[CK_MAT];
  const int t = threadIdx.x;
  if (mat < 0) {
    float* pp = p + start;
    const float* gg = g + start;
    float* mm = m + start;
    float* vv = v + start;
    int done = 0;
    if (((((uintptr_t)pp | (uintptr_t)gg | (uintptr_t)mm | (uintptr_t)vv)) & 15) == 0) {
      const int n4 = len / 4;
      for (int i = t; i < n4; i += MU_THREADS) {
        float4 a = ((float4*)pp)[i], c = ((float4*)mm)[i], d = ((float4*)vv)[i];
        const float4 b = ((const float4*)gg)[i];
        mu_adamw_elem(a.x, b.x, c.x, d.x, s);
        mu_adamw_elem(a.y, b.y, c.y, d.y, s);
        mu_adamw_elem(a.z, b.z, c.z, d.z, s);
        mu_adamw_elem(a.w, b.w, c.w, d.w, s);
        ((float4*)pp)[i] = a;
        ((float4*)mm)[i] = c;
        ((float4*)vv)[i] = d;
      }
      done = n4 * 4;
    }
    for (int i = done + t; i < len; i += MU_THREADS) {
      float a = pp[i], c = mm[i], d = vv[i];
      mu_adamw_elem(a, gg[i], c, d, s);
      pp[i] = a;
      mm[i] = c;
      vv[i] = d;
    }
    return;
  }
  const int64_t* e = mu_row(mats, mat);
  const float* gg = g + start;
  float* mm = m + start;
  bf16_t* xx = xws + e[MT_XOFF] + (start - e[MT_OFF]);
  float acc = 0.0f;
  int done = 0;
  if (((((uintptr_t)gg | (uintptr_t)mm)) & 15) == 0 && ((uintptr_t)xx & 7) == 0) {
    const int n4 = len / 4;
    for (int i = t; i < n4; i += MU_THREADS) {
      const float4 b = ((const float4*)gg)[i];
      float4 c = ((float4*)mm)[i];
      bf16_t u0, u1, u2, u3;
      const float f0 = mu_muon_elem(b.x, c.x, s, u0), f1 = mu_muon_elem(b.y, c.y, s, u1);
      const float f2 = mu_muon_elem(b.z, c.z, s, u2), f3 = mu_muon_elem(b.w, c.w, s, u3);
      ((float4*)mm)[i] = c;
      u32x2_t pk;
      pk[0] = (uint32_t)u0 | ((uint32_t)u1 << 16);
      pk[1] = (uint32_t)u2 | ((uint32_t)u3 << 16);
      ((u32x2_t*)xx)[i] = pk;
      acc = fmaf(f0, f0, acc);
      acc = fmaf(f1, f1, acc);
      acc = fmaf(f2, f2, acc);
      acc = fmaf(f3, f3, acc);
    }
    done = n4 * 4;
  }
  for (int i = done + t; i < len; i += MU_THREADS) {
    float c = mm[i];
    bf16_t u;
    const float f = mu_muon_elem(gg[i], c, s, u);
    mm[i] = c;
    xx[i] = u;
    acc = fmaf(f, f, acc);
  }
  const float tot = mu_block_sum(acc, wsum);
  if (t == 0) partials[blockIdx.x] = tot;
}

extern "C" int dl_muon_pre(float* p, const float* g, float* m, float* v, int64_t n, const int64_t* chunks_host,
                           const int64_t* chunks_dev, int64_t n_chunks, const int64_t* mats_host, const int64_t* mats_dev,
                           int64_t n_mat, void* xws, int64_t x_cap, float* partials, int64_t partials_cap, float lr, float beta1,
                           float beta2, float eps, float weight_decay, float bias_corr1, float bias_corr2, float momentum,
                           float grad_scale, const float* coef, int nesterov, dl_stream_t stream) {
  DL_CHECK_ARG(p && g && m && n > 0 && chunks_host && chunks_dev && n_chunks > 0 && n_chunks < (1ll << 31), "dl_muon_pre: bad args");
  DL_CHECK_ARG(((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)coef | (uintptr_t)partials)) & 3) == 0,
               "dl_muon_pre: 4B alignment");
  DL_CHECK_ARG(n_mat == 0 || (xws && partials && partials_cap >= n_chunks && ((uintptr_t)xws & 15) == 0),
               "dl_muon_pre: Muon matrices need the X workspace (16B aligned) and one partials slot per chunk");
  DL_CHECK_ARG(momentum >= 0.0f, "dl_muon_pre: momentum %g < 0", (double)momentum);
  const int rc = mu_check_mats("dl_muon_pre", mats_host, mats_dev, n_mat, n, x_cap, INT64_MAX);
  if (rc != DL_OK) return rc;
  // the chunks tile [0, n) in order, each inside one matrix or outside all of them
  int64_t at = 0, im = 0;
  for (int64_t c = 0; c < n_chunks; ++c) {
    const int64_t* ck = chunks_host + c * DL_MUON_CHUNK_FIELDS;
    const int64_t s0 = ck[CK_START], len = ck[CK_LEN], mat = ck[CK_MAT];
    DL_CHECK_ARG(s0 == at && len > 0 && len <= DL_MUON_CHUNK && s0 + len <= n && mat >= -1 && mat < n_mat,
                 "dl_muon_pre: chunk %lld (start %lld, length %lld, matrix %lld) breaks the chunk order or leaves the buffer", (long long)c,
                 (long long)s0, (long long)len, (long long)mat);
    while (im < n_mat && mats_host[im * DL_MUON_MAT_FIELDS + MT_OFF] + mats_host[im * DL_MUON_MAT_FIELDS + MT_ROWS] * mats_host[im * DL_MUON_MAT_FIELDS + MT_COLS] <= s0) ++im;
    const int64_t* e = mats_host + im * DL_MUON_MAT_FIELDS;
    const bool inside = im < n_mat && s0 >= e[MT_OFF];
    if (inside) {
      DL_CHECK_ARG(mat == im && s0 + len <= e[MT_OFF] + e[MT_ROWS] * e[MT_COLS] && c >= e[MT_CHUNK0] && c < e[MT_CHUNK0] + e[MT_NCHUNK],
                   "dl_muon_pre: chunk %lld does not lie in the chunk range of matrix %lld", (long long)c, (long long)im);
    } else {
      DL_CHECK_ARG(mat == -1 && (im >= n_mat || s0 + len <= e[MT_OFF]), "dl_muon_pre: auxiliary chunk %lld overlaps a Muon matrix",
                   (long long)c);
      DL_CHECK_ARG(v, "dl_muon_pre: auxiliary ranges need the second moment");
    }
    at = s0 + len;
  }
  DL_CHECK_ARG(at == n, "dl_muon_pre: the chunks cover %lld of %lld elements", (long long)at, (long long)n);
  MuPre s;
  s.lr = lr, s.b1 = beta1, s.b2 = beta2, s.eps = eps, s.wd = weight_decay;
  s.inv_bc1_lr = (float)((double)lr / (double)bias_corr1);
  s.inv_sqrt_bc2 = (float)(1.0 / sqrt((double)bias_corr2));
  s.w1 = (float)(1.0 - (double)momentum), s.mom = momentum, s.gs = grad_scale, s.nesterov = nesterov != 0;
  hipLaunchKernelGGL(muon_pre_k, (int)n_chunks, MU_THREADS, 0, (hipStream_t)stream, p, g, m, v, chunks_dev, mats_dev, (bf16_t*)xws,
                     partials, s, coef);
  DL_LAUNCH_CHECK();
  return DL_OK;
}

// ---------------------------------------------------------------- fold: norms[i] = max(||bf16(U_i)||_F, eps)
__global__ __launch_bounds__(MU_THREADS) void muon_fold_k(const int64_t* __restrict__ mats, const float* __restrict__ partials, float eps,
                                                           float* __restrict__ norms) {
  __shared__ double red[MU_THREADS];
  const int64_t* e = mu_row(mats, blockIdx.x);
  const int64_t c0 = e[MT_CHUNK0], n_slots = e[MT_NCHUNK];
  const int64_t per = (n_slots + MU_THREADS - 1) / MU_THREADS;
  const int64_t lo = (int64_t)threadIdx.x * per;
  const int64_t hi = lo + per < n_slots ? lo + per : n_slots;
  double s = 0.0;
  for (int64_t i = lo; i < hi; ++i) s += (double)partials[c0 + i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = 1; w < MU_THREADS; w <<= 1) {
    if ((threadIdx.x & (2 * w - 1)) == 0) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float nrm = (float)sqrt(red[0]);
    norms[blockIdx.x] = nrm < eps ? eps : nrm;  // (a NaN norm stays NaN, as torch's clamp leaves it)
  }
}

// ---------------------------------------------------------------- stage: X = bf16(X / norm) in place, 4096 elements per workgroup
__global__ __launch_bounds__(MU_THREADS) void muon_stage_k(const int64_t* __restrict__ mats, int n_mat, const float* __restrict__ norms,
                                                            bf16_t* __restrict__ xws) {
  const int mat = mu_find(mats, n_mat, MT_AP0, blockIdx.x);
  const int64_t* e = mu_row(mats, mat);
  u32x4_t* x = (u32x4_t*)(xws + e[MT_XOFF] + ((int64_t)blockIdx.x - e[MT_AP0]) * MU_FLAT);
  const float nrm = norms[mat];
#pragma unroll
  for (int i = 0; i < MU_FLAT / 8 / MU_THREADS; ++i) {
    float f[8];
    unpack8(x[i * MU_THREADS + threadIdx.x], f);
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = f[j] / nrm;
    x[i * MU_THREADS + threadIdx.x] = pack8(f);
  }
}

// ---------------------------------------------------------------- grouped 64 x 64 tile GEMM: C = bf16(beta * D + alpha * opA opB^T)
// opA [64 of M, K] and opB [64 of N, K] as seen by the product; in memory an operand is contraction-contiguous (element (i, k) at
// i * ld + k) or contraction-strided (k * ld + i).  Four waves, wave w owns rows 16 w .. 16 w + 15 of the tile and all 64 columns:
// four 16x16x32 accumulators.  The MFMA is issued with the operands swapped (D^T = opB opA^T), so that a lane's four accumulator
// registers are four CONSECUTIVE columns of one row of C: one 8-byte store per accumulator.
struct MuOperand {
  const bf16_t* base;
  int64_t ld;
  int kstrided;
};
__device__ __forceinline__ void mu_stage_operand(const MuOperand& o, int64_t i0, int64_t k0, bf16_t (*lds)[MU_LDS_LD]) {
  const int t = threadIdx.x;
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int a = t / 8 + 32 * r, c8 = (t % 8) * 8;
    if (!o.kstrided) {  // row a of the tile, contraction elements c8 .. c8 + 7
      *(u32x4_t*)&lds[a][c8] = *(const u32x4_t*)(o.base + (i0 + a) * o.ld + k0 + c8);
    } else {  // contraction row a, tile rows c8 .. c8 + 7: transposed into the LDS
      const u32x4_t q = *(const u32x4_t*)(o.base + (k0 + a) * o.ld + i0 + c8);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        lds[c8 + 2 * j][a] = (bf16_t)(q[j] & 0xffffu);
        lds[c8 + 2 * j + 1][a] = (bf16_t)(q[j] >> 16);
      }
    }
  }
}
__device__ __forceinline__ void mu_tile(const MuOperand& A, const MuOperand& B, int64_t K, int64_t tm, int64_t tn,
                                        const bf16_t* __restrict__ D, bf16_t* __restrict__ C, int64_t ldc, float alpha, float beta,
                                        bf16_t (*As)[MU_LDS_LD], bf16_t (*Bs)[MU_LDS_LD]) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  f32x4_t acc[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) acc[c] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  for (int64_t k0 = 0; k0 < K; k0 += MU_BK) {
    mu_stage_operand(A, tm * MU_TILE, k0, As);
    mu_stage_operand(B, tn * MU_TILE, k0, Bs);
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < MU_BK / 32; ++ks) {
      const bf16x8_t af = *(const bf16x8_t*)&As[16 * w + (lane & 15)][32 * ks + 8 * (lane >> 4)];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const bf16x8_t bfr = *(const bf16x8_t*)&Bs[16 * c + (lane & 15)][32 * ks + 8 * (lane >> 4)];
        acc[c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr, af, acc[c], 0, 0, 0);
      }
    }
    __syncthreads();
  }
  // lane: row 16 w + (lane & 15) of the tile, columns 16 c + 4 (lane >> 4) + {0, 1, 2, 3}
  const int64_t row = tm * MU_TILE + 16 * w + (lane & 15);
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int64_t col = tn * MU_TILE + 16 * c + 4 * (lane >> 4);
    float o[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) o[r] = alpha * acc[c][r];
    if (D) {
      const u32x2_t d = *(const u32x2_t*)(D + row * ldc + col);
      o[0] = fmaf(beta, bflo(d[0]), o[0]);
      o[1] = fmaf(beta, bfhi(d[0]), o[1]);
      o[2] = fmaf(beta, bflo(d[1]), o[2]);
      o[3] = fmaf(beta, bfhi(d[1]), o[3]);
    }
    u32x2_t q;
    q[0] = pack2bf(o[0], o[1]);
    q[1] = pack2bf(o[2], o[3]);
    *(u32x2_t*)(C + row * ldc + col) = q;
  }
}

enum { MU_GRAM = 0, MU_POLY = 1, MU_APPLY = 2 };
template <int PHASE>
__global__ __launch_bounds__(MU_THREADS) void muon_gemm_k(const int64_t* __restrict__ mats, int n_mat, const bf16_t* __restrict__ xin,
                                                           bf16_t* __restrict__ xout, bf16_t* __restrict__ aws,
                                                           bf16_t* __restrict__ pws, float alpha, float beta) {
  __shared__ __attribute__((aligned(16))) bf16_t As[MU_TILE][MU_LDS_LD];
  __shared__ __attribute__((aligned(16))) bf16_t Bs[MU_TILE][MU_LDS_LD];
  const int mat = mu_find(mats, n_mat, PHASE == MU_APPLY ? MT_AP0 : MT_SQ0, blockIdx.x);
  const int64_t* e = mu_row(mats, mat);
  const int64_t rows = e[MT_ROWS], cols = e[MT_COLS];
  const bool tall = rows > cols;
  const int64_t ms = tall ? cols : rows, ml = tall ? rows : cols;
  const int64_t t = (int64_t)blockIdx.x - e[PHASE == MU_APPLY ? MT_AP0 : MT_SQ0];
  const bf16_t* X = xin + e[MT_XOFF];
  bf16_t* Am = aws + e[MT_AOFF];
  bf16_t* Pm = pws + e[MT_AOFF];
  if (PHASE == MU_GRAM) {  // A = X X^T (wide) or X^T X (tall): [ms, ms], contraction over the long dimension
    const MuOperand x = {X, cols, tall};
    mu_tile(x, x, ml, t / (ms / MU_TILE), t % (ms / MU_TILE), nullptr, Am, ms, 1.0f, 0.0f, As, Bs);
  } else if (PHASE == MU_POLY) {  // P = b A + c A A; A is symmetric, so its rows serve as the columns of the second factor
    const MuOperand a = {Am, ms, 0};
    mu_tile(a, a, ms, t / (ms / MU_TILE), t % (ms / MU_TILE), Am, Pm, ms, alpha, beta, As, Bs);
  } else {  // X' = a X + P X (wide: X enters contraction-strided) or a X + X P (tall: P symmetric, read by rows)
    const MuOperand pm = {Pm, ms, 0};
    const MuOperand xa = {X, cols, 0}, xb = {X, cols, 1};
    mu_tile(tall ? xa : pm, tall ? pm : xb, ms, t / (cols / MU_TILE), t % (cols / MU_TILE), X, xout + e[MT_XOFF], cols, alpha, beta, As,
            Bs);
  }
}

extern "C" int dl_muon_orthogonalize(const int64_t* mats_host, const int64_t* mats_dev, int64_t n_mat, const float* partials,
                                     float* norms, void* xws, int64_t x_cap, void* aws, int64_t a_cap, float eps, float a, float b,
                                     float c, int ns_steps, dl_stream_t stream) {
  DL_CHECK_ARG(mats_host && mats_dev && n_mat > 0 && partials && norms && xws && aws, "dl_muon_orthogonalize: bad args");
  DL_CHECK_ARG(ns_steps >= 0 && ns_steps < MU_MAX_STEPS, "dl_muon_orthogonalize: ns_steps %d outside [0, %d)", ns_steps, MU_MAX_STEPS);
  DL_CHECK_ARG(((((uintptr_t)xws | (uintptr_t)aws)) & 15) == 0 && ((((uintptr_t)partials | (uintptr_t)norms)) & 3) == 0,
               "dl_muon_orthogonalize: the workspaces must be 16B aligned");
  DL_CHECK_ARG(x_cap > 0 && a_cap > 0 && x_cap % 8 == 0 && a_cap % 8 == 0, "dl_muon_orthogonalize: workspace capacities");
  // xws holds two copies of X (x_cap elements each), aws holds A and P (a_cap elements each)
  const int rc = mu_check_mats("dl_muon_orthogonalize", mats_host, mats_dev, n_mat, INT64_MAX, x_cap, a_cap);
  if (rc != DL_OK) return rc;
  const int64_t* tot = mats_host + n_mat * DL_MUON_MAT_FIELDS;
  const int sq = (int)tot[MT_SQ0], ap = (int)tot[MT_AP0], nm = (int)n_mat;
  hipStream_t st = (hipStream_t)stream;
  bf16_t* x[2] = {(bf16_t*)xws, (bf16_t*)xws + x_cap};
  bf16_t* am = (bf16_t*)aws;
  bf16_t* pm = (bf16_t*)aws + a_cap;
  int launches = 0;
  hipLaunchKernelGGL(muon_fold_k, nm, MU_THREADS, 0, st, mats_dev, partials, eps, norms);
  DL_LAUNCH_CHECK();
  hipLaunchKernelGGL(muon_stage_k, ap, MU_THREADS, 0, st, mats_dev, nm, norms, x[0]);
  DL_LAUNCH_CHECK();
  launches += 2;
  for (int s = 0; s < ns_steps; ++s) {
    hipLaunchKernelGGL(muon_gemm_k<MU_GRAM>, sq, MU_THREADS, 0, st, mats_dev, nm, x[s & 1], x[(s + 1) & 1], am, pm, 1.0f, 0.0f);
    DL_LAUNCH_CHECK();
    hipLaunchKernelGGL(muon_gemm_k<MU_POLY>, sq, MU_THREADS, 0, st, mats_dev, nm, x[s & 1], x[(s + 1) & 1], am, pm, c, b);
    DL_LAUNCH_CHECK();
    hipLaunchKernelGGL(muon_gemm_k<MU_APPLY>, ap, MU_THREADS, 0, st, mats_dev, nm, x[s & 1], x[(s + 1) & 1], am, pm, 1.0f, a);
    DL_LAUNCH_CHECK();
    launches += 3;
  }
  return launches;
}

// ---------------------------------------------------------------- post pass: p = p (1 - lr wd) - lr ratio O
__global__ __launch_bounds__(MU_THREADS) void muon_post_k(float* __restrict__ p, const int64_t* __restrict__ mats, int n_mat,
                                                           const bf16_t* __restrict__ xo, float decay, float lr) {
#pragma clang fp contract(off)
  const int mat = mu_find(mats, n_mat, MT_AP0, blockIdx.x);
  const int64_t* e = mu_row(mats, mat);
  const int64_t local = ((int64_t)blockIdx.x - e[MT_AP0]) * MU_FLAT;
  const bf16_t* o = xo + e[MT_XOFF] + local;
  float* pp = p + e[MT_OFF] + local;
  const float alr = lr * __uint_as_float((uint32_t)e[MT_RATIO]);
  if (((uintptr_t)pp & 15) == 0) {
#pragma unroll
    for (int i = 0; i < MU_FLAT / 4 / MU_THREADS; ++i) {
      const int q = i * MU_THREADS + threadIdx.x;
      const u32x2_t ob = ((const u32x2_t*)o)[q];
      float4 w = ((float4*)pp)[q];
      w.x = w.x * decay - alr * bflo(ob[0]);
      w.y = w.y * decay - alr * bfhi(ob[0]);
      w.z = w.z * decay - alr * bflo(ob[1]);
      w.w = w.w * decay - alr * bfhi(ob[1]);
      ((float4*)pp)[q] = w;
    }
  } else {
    for (int i = threadIdx.x; i < MU_FLAT; i += MU_THREADS) pp[i] = pp[i] * decay - alr * bf2f(o[i]);
  }
}

extern "C" int dl_muon_post(float* p, int64_t n, const int64_t* mats_host, const int64_t* mats_dev, int64_t n_mat, const void* xo,
                            int64_t x_cap, float lr, float weight_decay, dl_stream_t stream) {
  DL_CHECK_ARG(p && n > 0 && mats_host && mats_dev && n_mat > 0 && xo, "dl_muon_post: bad args");
  DL_CHECK_ARG(((uintptr_t)p & 3) == 0 && ((uintptr_t)xo & 15) == 0, "dl_muon_post: p 4B aligned, O 16B aligned");
  const int rc = mu_check_mats("dl_muon_post", mats_host, mats_dev, n_mat, n, x_cap, INT64_MAX);
  if (rc != DL_OK) return rc;
  const float decay = (float)(1.0 - (double)lr * (double)weight_decay);
  hipLaunchKernelGGL(muon_post_k, (int)mats_host[n_mat * DL_MUON_MAT_FIELDS + MT_AP0], MU_THREADS, 0, (hipStream_t)stream, p, mats_dev,
                     (int)n_mat, (const bf16_t*)xo, decay, lr);
  DL_LAUNCH_CHECK();
  return DL_OK;
}
