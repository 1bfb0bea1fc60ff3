// Activation-stationary NT GEMMs for a short contraction (K <= 512) and a wide output: the forward MLP-up GEMM with the fused SwiGLU
// (dl_gemm_nt_swiglu_stationary) and the qkv GEMM with the QK-norm statistics (dl_gemm_nt_ssq_stationary).
//
// gemm_nt_big_k (gemm.hip) stages a 256-row activation panel through LDS once per column tile: at K = 384 and N = 3072 the same panel
// passes the LDS eight times, next to 384 weight rows each time, and every tile restarts the load / MFMA / store sequence of a workgroup
// that owns its CU.  Here the panel never touches LDS:
//   * one 512-thread workgroup per CU owns a 256-row panel; wave w keeps rows 32w .. 32w+31 of it in registers for the whole panel, as
//     the K/16 B-operand fragments of v_mfma_f32_32x32x16_bf16 (96 VGPRs at K = 384), loaded once from global memory in fragment layout;
//   * only the weight streams through LDS, as stages of 64 whole rows (64 x 2K bytes: full cache lines), through an NST-slot ring behind
//     counted s_waitcnt vmcnt waits and a raw s_barrier (the ring of gemm_nt_big_k); the stream never drains between column blocks,
//     and wraps to the first weight row when a capped workgroup goes on to its next panel;
//   * the LDS image is lane-linear (direct-to-LDS DMA), so the bank swizzle goes into the DMA's source address: within a row the 16-byte
//     slot index is XORed with row & 15 (row pitch a multiple of 256 bytes) or with (row >> 1) & 7 (pitch = 128 mod 256), which puts the
//     16 rows of every ds_read_b128 lane group on 64 distinct banks;
//   * every wave computes its 32 rows of all N columns, two 32-column blocks (one stage) at a time into ping-pong accumulators: the
//     waves share no output tile, and the epilogue of a stage runs at opposite ends of the stage on the two waves of a SIMD, so one
//     wave's epilogue arithmetic runs under the other wave's MFMAs (measured against four blocks per epilogue on every wave at the
//     same point: 157 -> 155 us at the MLP-up shape, 142 with the explicit LDS waits below).
// Every output element is ONE accumulator chain over ascending k of mfma(w_frag, x_frag, acc) -- operand order and summation order of
// gemm_nt_big_k -- and the epilogues repeat nt_epilogue_regs<.., 2> / nt_epilogue_ssq on the unrounded accumulators: U, H and C are
// bit-identical to dl_gemm_nt_swiglu / dl_gemm_nt_ssq.  The row sums of squares are wave-local here (a wave owns whole rows): plain
// stores instead of two atomic addends, summed in the grouping of nt_epilogue_ssq (192 columns per lane half, the halves, then the two
// 192-column sums), so they too carry the bits of dl_gemm_nt_ssq, and do not need the caller's zero fill.
#include <stdlib.h>

#include <type_traits>

#include "common.h"
#include "gemm_paths.h"
#include "gemm_stationary_body.h"

// workgroup g of G walks the panels g, g + G, ... (g < panels by launch); the body is st_gemm_body (gemm_stationary_body.h)
template <int NKS, int EPI>
__global__ __launch_bounds__(ST_THREADS) void gemm_nt_stationary_k(StArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int panels = a.M / ST_PANEL, G = gridDim.x;
  st_gemm_body<NKS, EPI>(a, smem, (int)threadIdx.x, (int)blockIdx.x, G, (panels - (int)blockIdx.x + G - 1) / G);
}

// grid of a launch, or 0 when the shape is not served: K % 64 == 0 up to 512, whole 256-row panels, whole groups of 128 columns.
// max_workgroups == 0: one workgroup per CU of the budget of the enclosing DlWgCapScope, and -- the rule of dispatch_big -- the panels
// must fill at least 0.7 of their rounds on it.  max_workgroups > 0: the caller sized the grid (still bounded by that budget) and its
// workgroups loop over the panels, however many rounds that takes.
static int st_grid(int64_t M, int64_t N, int64_t K, int max_workgroups, int n_cu) {
  if (K % 64 || K > 512 || M % ST_PANEL || N % 128) return 0;
  const int64_t panels = M / ST_PANEL;
  int64_t g = dl_wg_budget(n_cu);
  if (max_workgroups > 0) {
    if (max_workgroups < g) g = max_workgroups;
  } else {
    const int64_t rounds = (panels + g - 1) / g;
    if ((double)panels < 0.7 * (double)(rounds * g)) return 0;
  }
  return (int)(g < panels ? g : panels);
}

template <int NKS, int EPI>
static void st_launch_nks(int grid, const StArgs& a, hipStream_t stream) {
  constexpr int STAGE = ST_ROWS * NKS * 128;
  constexpr int LDS = ((3 * STAGE <= 160 * 1024) ? 3 : 2) * STAGE;
  static DevOnce once;
  (void)dev_cus(once, [] {
    (void)hipFuncSetAttribute((const void*)gemm_nt_stationary_k<NKS, EPI>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS);
  });
  hipLaunchKernelGGL((gemm_nt_stationary_k<NKS, EPI>), grid, ST_THREADS, LDS, stream, a);
}
template <int EPI>
static int st_launch(int grid, int64_t K, const StArgs& a, hipStream_t stream) {
  dl_note_path(DL_PATH_NONE);  // no code of its own in enum DlGemmPath
  switch (K / 64) {
    case 1: st_launch_nks<1, EPI>(grid, a, stream); break;
    case 2: st_launch_nks<2, EPI>(grid, a, stream); break;
    case 3: st_launch_nks<3, EPI>(grid, a, stream); break;
    case 4: st_launch_nks<4, EPI>(grid, a, stream); break;
    case 5: st_launch_nks<5, EPI>(grid, a, stream); break;
    case 6: st_launch_nks<6, EPI>(grid, a, stream); break;
    case 7: st_launch_nks<7, EPI>(grid, a, stream); break;
    default: st_launch_nks<8, EPI>(grid, a, stream); break;
  }
  DL_LAUNCH_CHECK();
  return DL_OK;
}
static int st_cus() {
  static DevOnce once;
  return dev_cus(once, [] {});
}

extern "C" int dl_gemm_nt_swiglu_stationary(const void* X, int64_t ldx, const void* Wp, int64_t ldw, void* U, int64_t ldu, void* H,
                                            int64_t ldh, int64_t M, int64_t F, int64_t K, int max_workgroups, dl_stream_t stream) {
  DL_CHECK_ARG(X && Wp && H && M > 0 && F > 0 && K > 0, "dl_gemm_nt_swiglu_stationary: null/empty operand");  // U may be NULL
  DL_CHECK_ARG(ldx % 8 == 0 && ldw % 8 == 0 && (!U || ldu % 8 == 0) && ldh % 8 == 0 && ldx >= K && ldw >= K && (!U || ldu >= 2 * F) &&
                   ldh >= F && ldw < (1ll << 24) && max_workgroups >= 0,
               "dl_gemm_nt_swiglu_stationary: leading dims (ldx=%lld ldw=%lld ldu=%lld ldh=%lld)", (long long)ldx, (long long)ldw,
               (long long)ldu, (long long)ldh);
  DL_CHECK_ARG((((uintptr_t)X | (uintptr_t)Wp | (uintptr_t)U | (uintptr_t)H) & 15) == 0 && M < (1ll << 31) && F < (1ll << 30),
               "dl_gemm_nt_swiglu_stationary: 16-byte alignment / dims");
  const int grid = st_grid(M, 2 * F, K, max_workgroups, st_cus());
  if (grid <= 0) {
    dl_set_error("dl_gemm_nt_swiglu_stationary: needs K %% 64 == 0 up to 512, M %% 256 == 0, F %% 64 == 0 and panels for 0.7 of the CUs "
                 "(M=%lld F=%lld K=%lld)", (long long)M, (long long)F, (long long)K);
    return DL_ERR_UNSUPPORTED;
  }
  StArgs a{(const bf16_t*)X, ldx, (const bf16_t*)Wp, ldw, (bf16_t*)U, ldu, (bf16_t*)H, ldh, (int)F, nullptr, 0, (int)M, (int)(2 * F)};
  return st_launch<0>(grid, K, a, (hipStream_t)stream);
}

extern "C" int dl_gemm_nt_ssq_stationary(const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc, int64_t M,
                                         int64_t N, int64_t K, float* ssq, int64_t ssq_tiles, int max_workgroups, dl_stream_t stream) {
  DL_CHECK_ARG(A && B && C && ssq && M > 0 && N > 0 && K > 0, "dl_gemm_nt_ssq_stationary: null/empty operand");
  DL_CHECK_ARG(lda % 8 == 0 && ldb % 8 == 0 && ldc % 8 == 0 && lda >= K && ldb >= K && ldc >= N && ldb < (1ll << 24) && max_workgroups >= 0,
               "dl_gemm_nt_ssq_stationary: leading dims (lda=%lld ldb=%lld ldc=%lld)", (long long)lda, (long long)ldb, (long long)ldc);
  DL_CHECK_ARG((((uintptr_t)A | (uintptr_t)B | (uintptr_t)C) & 15) == 0 && ((uintptr_t)ssq & 3) == 0 && ssq_tiles >= 1 &&
                   ssq_tiles <= N / 384 + 1 && M < (1ll << 31) && N < (1ll << 31),
               "dl_gemm_nt_ssq_stationary: alignment / ssq_tiles / dims");
  const int grid = st_grid(M, N, K, max_workgroups, st_cus());
  if (grid <= 0) {
    dl_set_error("dl_gemm_nt_ssq_stationary: needs K %% 64 == 0 up to 512, M %% 256 == 0, N %% 128 == 0 and panels for 0.7 of the CUs "
                 "(M=%lld N=%lld K=%lld)", (long long)M, (long long)N, (long long)K);
    return DL_ERR_UNSUPPORTED;
  }
  StArgs a{(const bf16_t*)A, lda, (const bf16_t*)B, ldb, (bf16_t*)C, ldc, nullptr, 0, 0, ssq, (int)ssq_tiles, (int)M, (int)N};
  return st_launch<1>(grid, K, a, (hipStream_t)stream);
}
