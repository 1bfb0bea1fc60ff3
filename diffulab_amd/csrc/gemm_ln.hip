// Row-complete GEMMs: C[M, 384-wide tiles] = A[M,K] . W[*,K]^T on persistent 256 x 384 tiles whose EPILOGUE is a row kernel.
//
// At D = 384 a 256 x 384 output tile holds WHOLE rows, and with 256 tokens per sample it holds one whole sample.  So the
// HBM-bound row kernels that used to run between the GEMMs of a DiT block (round-2 profile: 6.9 of 22.7 ms per step) can run on
// the tile while it is still on chip -- the GEMM result never makes the round trip through HBM and the launches disappear:
//   RK_LNF  projection / MLP-down / patch-embedding GEMM  ->  x += gate * t ; LayerNorm ; modulate       (mmdit.py:296-308, nn.py:539)
//           writes t (kept for the gate gradient), the new residual stream x, the modulated rows xm and the row statistics
//   RK_LNB  the two N = D data-gradient GEMMs (K = 3D and 2F) and the head's ->  LayerNorm-modulate backward + the backward of the
//           gated residual that follows in the chain; the per-sample column sums (dscale, dshift, dgate, LayerNorm-affine
//           partials) are COMPLETE inside the tile: plain stores, no atomics, a fixed summation order (deterministic)
//   RK_QK   qkv GEMM (N = 3D: tile 0 = q, 1 = k, 2 = v)  ->  RMSNorm over the full 384-wide q / k row, RoPE, head-major store
//           (mmdit.py:81-91, nn.py:345-352,430); the pre-norm qkv rows are still written (the backward and the in-place V need them)
//
// Main loop: the 256 x 384 walk of gemm_nt_big_k (gemm.hip): 8 waves as 4 (M) x 2 (N), each 64 x 192 = 2 x 6 MFMA 32x32x16 tiles,
// 64-deep k-steps DMA'd straight into a two-slot LDS ring (80 KiB per slot), source-side XOR swizzle, operand-swapped MFMAs.
//
// Epilogue = "the row kernel, fed from LDS": the accumulators are rounded to bf16 (exactly what the unfused GEMM would have
// stored), dumped 64 rows at a time into the LDS slot the last k-step has just released (row pitch 784 B: consecutive rows
// shift by four banks, the 16-byte writes of eight lanes cover 32 banks), and then every wave owns a ROW: lane c holds columns
// [8c, 8c+8) -- the thread layout of norm.hip's kernels, the same DPP wave sums in the same order, so t, x and qkv are
// BIT-IDENTICAL to the unfused launch sequence and the statistics and the rows computed from them agree with it to their last
// bits (tests/test_row_gemm_gpu.py; tests/test_row_gemm_paths_gpu.py checks every output element against fp64), and per-sample
// column sums are plain in-lane accumulators over the tile's rows.  Global operands of the row (x, dres, t / residual) are prefetched one row
// ahead; their rows are contiguous 768-byte segments per wave instruction.
#include <stdlib.h>

#include "common.h"
#include "gemm_rows_body.h"

// workgroup b of G (a multiple of 8, <= ntiles) takes slot (b & 7) * (G / 8) + (b >> 3) and walks the tiles slot, slot + G, ...;
// the body is rk_gemm_body (gemm_rows_body.h)
template <int MODE>
__global__ __launch_bounds__(RK_THREADS, 2) void gemm_nt_rows_k(const bf16_t* __restrict__ A, int64_t lda,
                                                                const bf16_t* __restrict__ Bm, int64_t ldb, int M, int N, int K,
                                                                RowEpi ep) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int ntiles = (M / RK_BM) * (N / RK_BN);
  const int G = gridDim.x;
  const int slot0 = (blockIdx.x & 7) * (G >> 3) + (blockIdx.x >> 3);
  rk_gemm_body<MODE>(A, lda, Bm, ldb, N, K, ep, smem, (int)threadIdx.x, slot0, G, (ntiles - slot0 + G - 1) / G);
}

template <int MODE>
static int rk_launch(const void* A, int64_t lda, const void* W, int64_t ldw, int64_t M, int64_t N, int64_t K, const RowEpi& ep,
                     hipStream_t stream) {
  constexpr int LDS = 2 * RK_STAGE;
  static DevOnce once;
  const int n_cu = dev_cus(once, [] {
    (void)hipFuncSetAttribute((const void*)gemm_nt_rows_k<MODE>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS);
  });
  const int ntiles = (int)((M / RK_BM) * (N / RK_BN));
  const int budget = dl_wg_budget(n_cu);
  int grid = budget < ntiles ? budget : ntiles;
  grid &= ~7;
  hipLaunchKernelGGL((gemm_nt_rows_k<MODE>), grid, RK_THREADS, LDS, stream, (const bf16_t*)A, lda, (const bf16_t*)W, ldw, (int)M,
                     (int)N, (int)K, ep);
  DL_LAUNCH_CHECK();
  return DL_OK;
}

// shapes the row-complete tiles serve: rows are exactly one tile wide, a modulation group is exactly one tile high
static bool rk_shape_ok(int64_t M, int64_t D, int64_t K, int64_t rows_per_mod) {
  return D == RK_BN && M % RK_BM == 0 && M / RK_BM >= 8 && K % RK_BK == 0 && K > 0 && rows_per_mod == RK_BM && M < (1ll << 31);
}
#define RK_ALIGNED16(p) ((((uintptr_t)(p)) & 15) == 0)

extern "C" int dl_ln_modulate_gemm_fwd(const void* A, int64_t lda, const void* W, int64_t ldw, int64_t M, int64_t K,
                                       const void* resid, const void* gate, int64_t ld_gate, const float* ln_w, const float* ln_b,
                                       const void* scale, const void* shift, int64_t ld_mod, int64_t rows_per_mod, float eps,
                                       void* t_out, void* x_out, void* xm_out, float* mean, float* rstd, int64_t D,
                                       dl_stream_t stream) {
  DL_CHECK_ARG(A && W && scale && shift && xm_out && mean && rstd && M > 0, "dl_ln_modulate_gemm_fwd: null operand");
  DL_CHECK_ARG((ln_w == nullptr) == (ln_b == nullptr), "dl_ln_modulate_gemm_fwd: w and b must both be given or both NULL");
  DL_CHECK_ARG(!gate || resid, "dl_ln_modulate_gemm_fwd: a gate needs the residual it gates into");
  DL_CHECK_ARG(!resid || x_out, "dl_ln_modulate_gemm_fwd: the updated residual stream needs x_out");
  if (!rk_shape_ok(M, D, K, rows_per_mod)) {
    dl_set_error("dl_ln_modulate_gemm_fwd: no row-complete tile for M=%lld D=%lld K=%lld rows_per_mod=%lld", (long long)M,
                 (long long)D, (long long)K, (long long)rows_per_mod);
    return DL_ERR_UNSUPPORTED;
  }
  DL_CHECK_ARG(lda % 8 == 0 && ldw % 8 == 0 && lda >= K && ldw >= K && ld_mod % 8 == 0 && (!gate || ld_gate % 8 == 0),
               "dl_ln_modulate_gemm_fwd: leading dimensions");
  DL_CHECK_ARG(RK_ALIGNED16(A) && RK_ALIGNED16(W) && RK_ALIGNED16(resid) && RK_ALIGNED16(gate) && RK_ALIGNED16(scale) &&
                   RK_ALIGNED16(shift) && RK_ALIGNED16(t_out) && RK_ALIGNED16(x_out) && RK_ALIGNED16(xm_out) && RK_ALIGNED16(ln_w) &&
                   RK_ALIGNED16(ln_b),
               "dl_ln_modulate_gemm_fwd: 16-byte alignment");
  RowEpi ep{};
  ep.resid = (const bf16_t*)resid;
  ep.gate = (const bf16_t*)gate;
  ep.ld_gate = ld_gate;
  ep.ln_w = ln_w;
  ep.ln_b = ln_b;
  ep.scale = (const bf16_t*)scale;
  ep.shift = (const bf16_t*)shift;
  ep.ld_mod = ld_mod;
  ep.eps = eps;
  ep.t_out = (bf16_t*)t_out;
  ep.x_out = (bf16_t*)x_out;
  ep.xm_out = (bf16_t*)xm_out;
  ep.mean = mean;
  ep.rstd = rstd;
  return rk_launch<RK_LNF>(A, lda, W, ldw, M, D, K, ep, (hipStream_t)stream);
}

extern "C" int dl_ln_modulate_gemm_bwd(const void* A, int64_t lda, const void* Wt, int64_t ldw, int64_t M, int64_t K,
                                       const void* x, const float* ln_w, const float* ln_b, const void* scale, int64_t ld_mod,
                                       int64_t rows_per_mod, const float* mean, const float* rstd, const void* dres, void* dx,
                                       float* dscale, float* dshift, int64_t ld_dmod, float* dwb, const void* gate_t,
                                       const void* gate, int64_t ld_gate, void* dt, float* dgate, int64_t D, dl_stream_t stream) {
  DL_CHECK_ARG(A && Wt && x && scale && mean && rstd && dx && dscale && dshift && M > 0, "dl_ln_modulate_gemm_bwd: null operand");
  DL_CHECK_ARG((ln_w == nullptr) == (ln_b == nullptr), "dl_ln_modulate_gemm_bwd: w and b must both be given or both NULL");
  DL_CHECK_ARG(!gate_t || (gate && dt && dgate), "dl_ln_modulate_gemm_bwd: the fused gate backward needs gate_t, gate, dt and dgate");
  if (!rk_shape_ok(M, D, K, rows_per_mod)) {
    dl_set_error("dl_ln_modulate_gemm_bwd: no row-complete tile for M=%lld D=%lld K=%lld rows_per_mod=%lld", (long long)M,
                 (long long)D, (long long)K, (long long)rows_per_mod);
    return DL_ERR_UNSUPPORTED;
  }
  DL_CHECK_ARG(lda % 8 == 0 && ldw % 8 == 0 && lda >= K && ldw >= K && ld_mod % 8 == 0 && (!gate_t || ld_gate % 8 == 0),
               "dl_ln_modulate_gemm_bwd: leading dimensions");
  DL_CHECK_ARG(RK_ALIGNED16(A) && RK_ALIGNED16(Wt) && RK_ALIGNED16(x) && RK_ALIGNED16(scale) && RK_ALIGNED16(dres) &&
                   RK_ALIGNED16(dx) && RK_ALIGNED16(gate_t) && RK_ALIGNED16(gate) && RK_ALIGNED16(dt) && RK_ALIGNED16(ln_w),
               "dl_ln_modulate_gemm_bwd: 16-byte alignment");
  RowEpi ep{};
  ep.x = (const bf16_t*)x;
  ep.ln_w = ln_w;
  ep.ln_b = ln_b;
  ep.scale = (const bf16_t*)scale;
  ep.ld_mod = ld_mod;
  ep.mean_i = mean;
  ep.rstd_i = rstd;
  ep.dres = (const bf16_t*)dres;
  ep.dx = (bf16_t*)dx;
  ep.dscale = dscale;
  ep.dshift = dshift;
  ep.ld_dmod = ld_dmod;
  ep.dwb = dwb;
  ep.gt = (const bf16_t*)gate_t;
  ep.gate = (const bf16_t*)gate;
  ep.ld_gate = ld_gate;
  ep.gdt = (bf16_t*)dt;
  ep.dgate = dgate;
  return rk_launch<RK_LNB>(A, lda, Wt, ldw, M, D, K, ep, (hipStream_t)stream);
}

extern "C" int dl_gemm_nt_qk_norm_rope(const void* A, int64_t lda, const void* Wqkv, int64_t ldw, int64_t B, int64_t N, int64_t H,
                                       int64_t dh, int64_t rot, float eps, const float* scale_q, const float* scale_k,
                                       const float* cos, const float* sin, void* qkv, void* q, void* k, float* rrms, int64_t n_dst,
                                       int64_t n_off, dl_stream_t stream) {
  DL_CHECK_ARG(A && Wqkv && scale_q && scale_k && cos && sin && qkv && q && k && rrms && B > 0 && N > 0,
               "dl_gemm_nt_qk_norm_rope: null operand");
  const int64_t D = H * dh, M = B * N;
  if (!rk_shape_ok(M, D, D, RK_BM) || dh % 8 || rot % 8 || rot > dh) {
    dl_set_error("dl_gemm_nt_qk_norm_rope: no row-complete tile for M=%lld D=%lld dh=%lld", (long long)M, (long long)D, (long long)dh);
    return DL_ERR_UNSUPPORTED;
  }
  DL_CHECK_ARG(n_off >= 0 && n_off + N <= n_dst, "dl_gemm_nt_qk_norm_rope: row window outside n_dst");
  DL_CHECK_ARG(lda % 8 == 0 && ldw % 8 == 0 && lda >= D && ldw >= D, "dl_gemm_nt_qk_norm_rope: leading dimensions");
  DL_CHECK_ARG(RK_ALIGNED16(A) && RK_ALIGNED16(Wqkv) && RK_ALIGNED16(qkv) && RK_ALIGNED16(q) && RK_ALIGNED16(k) &&
                   RK_ALIGNED16(scale_q) && RK_ALIGNED16(scale_k) && RK_ALIGNED16(cos) && RK_ALIGNED16(sin),
               "dl_gemm_nt_qk_norm_rope: 16-byte alignment");
  RowEpi ep{};
  ep.eps = eps;
  ep.qkv = (bf16_t*)qkv;
  ep.qo = (bf16_t*)q;
  ep.ko = (bf16_t*)k;
  ep.rrms = rrms;
  ep.sq = scale_q;
  ep.sk = scale_k;
  ep.cs = cos;
  ep.sn = sin;
  ep.n_tok = (int)N;
  ep.heads = (int)H;
  ep.dh = (int)dh;
  ep.rot = (int)rot;
  ep.n_dst = (int)n_dst;
  ep.n_off = (int)n_off;
  return rk_launch<RK_QK>(A, lda, Wqkv, ldw, M, 3 * D, D, ep, (hipStream_t)stream);
}
