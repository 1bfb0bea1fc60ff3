// dl_dit_block_fwd_chain: the forward of one adaLN-zero DiT block as ONE launch in which every workgroup carries whole samples through
// the block, phase after phase, with workgroup-local synchronisation only.
//
// At 256 tokens per sample and D = 384 every operation of the block's forward is local to a sample: a 256-row GEMM panel is a sample,
// LayerNorm / modulation / QK-norm / RoPE are per row or per sample, the attention is per sample.  The forward kernels of the
// row-complete path (gemm_stationary.hip, attention.hip, gemm_ln.hip) already share one shape -- 512 threads, one persistent workgroup
// per CU, workgroup p owns panel / sample p -- so the launch boundaries between them are grid-wide barriers the data flow does not
// need.  Here the same device bodies (gemm_stationary_body.h, attention_body.h, gemm_rows_body.h) run back to back: workgroup g walks
// the samples g, g + G, ... and runs, on that sample's panel only,
//   1. qkv GEMM + the QK-norm row statistics from the register-resident xm1 panel    (st_gemm_body<6, 1>)
//   2. QK-norm + RoPE on load + attention over the sample's heads                     (attn_qkn_pipe_body)
//   3. projection GEMM + the gated residual and LN2 + modulate as its row epilogue   (rk_gemm_body<RK_LNF>, K = D)
//   4. MLP-up GEMM + SwiGLU from the register-resident xm2 panel                      (st_gemm_body<6, 0>)
//   5. MLP-down GEMM + the gated residual and the NEXT LayerNorm + modulate           (rk_gemm_body<RK_LNF>, K = F)
// Between two phases the workgroup waits for all of its global stores (s_waitcnt vmcnt(0): stores on gfx950 count on vmcnt and are
// acknowledged by L2), fences at workgroup scope and meets at a barrier.  All waves of a workgroup run on one CU and share its vector
// L1, which is write-through and was invalidated at the launch, and no address a phase reads was read earlier in the launch: no cache
// action is needed.  No workgroup ever waits for another one: no grid-wide wait, no spinning on memory, no cooperative launch.
// Each output element is computed by the same instructions in the same order as in the separate launches: bit-identical results.
#include <stdlib.h>

#include "common.h"
#include "attention_body.h"
#include "gemm_rows_body.h"
#include "gemm_stationary_body.h"

#define CH_THREADS 512
#define CH_NKS 6  // D = 384 = 6 x 64

struct ChainRowGemm {
  const bf16_t* A;
  int64_t lda;
  const bf16_t* W;
  int64_t ldw;
  int K;
  RowEpi ep;
};
struct ChainAttn {
  const bf16_t* qkv;
  bf16_t* out;
  float* lse;
  int H;
  float scale;
  QkNorm qn;
};
struct ChainArgs {
  int B;
  StArgs qkv;
  ChainAttn attn;
  ChainRowGemm proj;
  StArgs up;
  ChainRowGemm down;
};

constexpr int ch_max(int a, int b) { return a > b ? a : b; }
constexpr int ch_lds_bytes() { return ch_max(ch_max(st_lds_bytes<CH_NKS>(), 2 * RK_STAGE), attn_pipe_lds_bytes(RK_BN)); }

// end of a phase: the operand rings are drained by their bodies; wait for this wave's stores, make them visible to the workgroup,
// and do not let any wave touch LDS or the phase's outputs before every wave is through
static __device__ __forceinline__ void ch_phase_sync() {
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __syncthreads();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// The arguments of a phase are read from the kernel-argument segment when the phase starts, through a pointer the compiler cannot
// see through: read once at the kernel's entry, the ~100 scalar registers of all phases stay live across every phase, spill into
// vector registers and push those into scratch inside the GEMM loops (196 bytes per lane, reloads in front of the counted waits).
// This way a phase holds what its stand-alone kernel holds.  (ChainArgs is the kernel's only parameter: offset 0 of the segment.)
static __device__ __forceinline__ const ChainArgs* ch_args() {
  auto p = __builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(p));
  return (const ChainArgs*)p;
}
// Likewise the thread index: what a phase derives from it (lane offsets of the operand rings, of the fragment reads, of the rows) would
// be computed once for all phases and held across them.
static __device__ __forceinline__ int ch_tid() {
  int t = threadIdx.x;
  asm volatile("" : "+v"(t));
  return t;
}
static __device__ __forceinline__ void ch_row_gemm(const ChainRowGemm* gp, char* smem, int sample) {
  const ChainRowGemm g = *gp;
  rk_gemm_body<RK_LNF>(g.A, g.lda, g.W, g.ldw, RK_BN, g.K, g.ep, smem, ch_tid(), sample, 0, 1);
}
template <int EPI>
static __device__ __forceinline__ void ch_st_gemm(const StArgs* ap, char* smem, int sample) {
  const StArgs a = *ap;
  st_gemm_body<CH_NKS, EPI>(a, smem, ch_tid(), sample, 0, 1);
}
static __device__ __forceinline__ void ch_attention(const ChainAttn* ap, char* smem, int sample) {
  const ChainAttn a = *ap;
  attn_qkn_pipe_body(a.qkv, a.out, a.lse, a.H, a.scale, a.qn, smem, ch_tid(), sample * a.H, 1, a.H);
}

__global__ __launch_bounds__(CH_THREADS, 2) void dit_block_fwd_chain_k(ChainArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  for (int s = blockIdx.x; s < a.B; s += gridDim.x) {
    ch_st_gemm<1>(&ch_args()->qkv, smem, s);
    ch_phase_sync();
    ch_attention(&ch_args()->attn, smem, s);
    ch_phase_sync();
    ch_row_gemm(&ch_args()->proj, smem, s);
    ch_phase_sync();
    ch_st_gemm<0>(&ch_args()->up, smem, s);
    ch_phase_sync();
    ch_row_gemm(&ch_args()->down, smem, s);
    ch_phase_sync();
  }
}

#define P(k) (b->p[DL_BLK_##k])
#define CH_ALIGNED16(p) ((((uintptr_t)(p)) & 15) == 0)

static void ch_row_epi(RowEpi& ep, const void* resid, const void* gate, int64_t ld_gate, const void* ln_w, const void* ln_b,
                       const void* scale, const void* shift, int64_t ld_mod, float eps, void* t_out, void* x_out, void* xm_out,
                       void* mean, void* rstd) {
  ep.resid = (const bf16_t*)resid;
  ep.gate = (const bf16_t*)gate;
  ep.ld_gate = ld_gate;
  ep.ln_w = (const float*)ln_w;
  ep.ln_b = (const float*)ln_b;
  ep.scale = (const bf16_t*)scale;
  ep.shift = (const bf16_t*)shift;
  ep.ld_mod = ld_mod;
  ep.eps = eps;
  ep.t_out = (bf16_t*)t_out;
  ep.x_out = (bf16_t*)x_out;
  ep.xm_out = (bf16_t*)xm_out;
  ep.mean = (float*)mean;
  ep.rstd = (float*)rstd;
}

extern "C" int dl_dit_block_fwd_chain(const dl_dit_block_t* b, int train, dl_stream_t stream) {
  DL_CHECK_ARG(b, "dl_dit_block_fwd_chain: null block");
  const int64_t B = b->B, N = b->N, D = b->D, H = b->H, F = b->F;
  DL_CHECK_ARG(B > 0 && N > 0 && D > 0 && H > 0 && F > 0, "dl_dit_block_fwd_chain: bad dims");
  if (!(b->row_gemms & 1) || !P(SSQ) || P(V) || N != RK_BM || D != RK_BN || D != H * 64 || F % 64 || F % RK_BK ||
      B * N >= (1ll << 31) || F >= (1ll << 30)) {
    dl_set_error("dl_dit_block_fwd_chain: needs row_gemms bit 0, SSQ, V in place, N == 256, D == 384, head_dim == 64, F %% 64 == 0 "
                 "(N=%lld D=%lld H=%lld F=%lld)", (long long)N, (long long)D, (long long)H, (long long)F);
    return DL_ERR_UNSUPPORTED;
  }
  DL_CHECK_ARG(P(XM1) && P(W_QKV) && P(QKV) && P(QN_SCALE) && P(KN_SCALE) && P(LSE) && (!train || (P(Q) && P(K) && P(RRMS))) &&
                   b->rot >= 0 && b->rot % 8 == 0 && b->rot <= 64 && (b->rot == 0 || (P(ROPE_COS) && P(ROPE_SIN))),
               "dl_dit_block_fwd_chain: null qkv / attention operand, or rot not a multiple of 8 up to 64");
  DL_CHECK_ARG(CH_ALIGNED16(P(XM1)) && CH_ALIGNED16(P(W_QKV)) && CH_ALIGNED16(P(QKV)) && CH_ALIGNED16(P(QN_SCALE)) && CH_ALIGNED16(P(KN_SCALE)) &&
                   CH_ALIGNED16(P(ROPE_COS)) && CH_ALIGNED16(P(ROPE_SIN)) && CH_ALIGNED16(P(Q)) && CH_ALIGNED16(P(K)) &&
                   (((uintptr_t)P(SSQ)) & 7) == 0,
               "dl_dit_block_fwd_chain: 16-byte alignment (qkv / attention operands)");
  DL_CHECK_ARG(P(A) && P(W_PROJ) && P(X_IN) && P(GATE1) && P(SCALE2) && P(SHIFT2) && P(T1) && P(X1) && P(XM2) && P(MEAN2) && P(RSTD2) &&
                   P(W_UP_PERM) && P(H) && P(W_DOWN) && P(GATE2) && P(T2) && P(NEXT_X) && P(NEXT_XM) && P(NEXT_SCALE) && P(NEXT_SHIFT) &&
                   P(NEXT_MEAN) && P(NEXT_RSTD),
               "dl_dit_block_fwd_chain: null operand");
  DL_CHECK_ARG((P(LN2_W) == nullptr) == (P(LN2_B) == nullptr) && (P(NEXT_LN_W) == nullptr) == (P(NEXT_LN_B) == nullptr),
               "dl_dit_block_fwd_chain: LayerNorm w and b must both be given or both NULL");
  DL_CHECK_ARG(b->ldw_d % 8 == 0 && b->ldw_f % 8 == 0 && b->ldw_d >= D && b->ldw_f >= F && b->ldw_d < (1ll << 24) && b->ld_mod % 8 == 0,
               "dl_dit_block_fwd_chain: leading dimensions");
  void* u = train ? P(U) : nullptr;
  DL_CHECK_ARG(CH_ALIGNED16(P(A)) && CH_ALIGNED16(P(W_PROJ)) && CH_ALIGNED16(P(X_IN)) && CH_ALIGNED16(P(GATE1)) && CH_ALIGNED16(P(SCALE2)) &&
                   CH_ALIGNED16(P(SHIFT2)) && CH_ALIGNED16(P(T1)) && CH_ALIGNED16(P(X1)) && CH_ALIGNED16(P(XM2)) && CH_ALIGNED16(P(LN2_W)) &&
                   CH_ALIGNED16(P(LN2_B)) && CH_ALIGNED16(P(W_UP_PERM)) && CH_ALIGNED16(u) && CH_ALIGNED16(P(H)) && CH_ALIGNED16(P(W_DOWN)) &&
                   CH_ALIGNED16(P(GATE2)) && CH_ALIGNED16(P(T2)) && CH_ALIGNED16(P(NEXT_X)) && CH_ALIGNED16(P(NEXT_XM)) &&
                   CH_ALIGNED16(P(NEXT_SCALE)) && CH_ALIGNED16(P(NEXT_SHIFT)) && CH_ALIGNED16(P(NEXT_LN_W)) && CH_ALIGNED16(P(NEXT_LN_B)),
               "dl_dit_block_fwd_chain: 16-byte alignment");

  ChainArgs a{};
  a.B = (int)B;
  a.qkv = StArgs{(const bf16_t*)P(XM1), D, (const bf16_t*)P(W_QKV), b->ldw_d, (bf16_t*)P(QKV), 3 * D, nullptr, 0, 0, (float*)P(SSQ), 2,
                 (int)(B * N), (int)(3 * D)};
  a.attn.qkv = (const bf16_t*)P(QKV);
  a.attn.out = (bf16_t*)P(A);
  a.attn.lse = (float*)P(LSE);
  a.attn.H = (int)H;
  a.attn.scale = 0.125f;  // 64^-0.5
  // (inference: the normalised q, k and rrms feed only the backward -- not written)
  a.attn.qn = QkNorm{(const float*)P(SSQ), (const float*)P(QN_SCALE), (const float*)P(KN_SCALE), (const float*)P(ROPE_COS),
                     (const float*)P(ROPE_SIN), (bf16_t*)(train ? P(Q) : nullptr), (bf16_t*)(train ? P(K) : nullptr),
                     (float*)(train ? P(RRMS) : nullptr), 1.0f / (float)D, 1e-6f, (int)b->rot, (int)(3 * D)};
  a.proj.A = (const bf16_t*)P(A);
  a.proj.lda = D;
  a.proj.W = (const bf16_t*)P(W_PROJ);
  a.proj.ldw = b->ldw_d;
  a.proj.K = (int)D;
  ch_row_epi(a.proj.ep, P(X_IN), P(GATE1), b->ld_mod, P(LN2_W), P(LN2_B), P(SCALE2), P(SHIFT2), b->ld_mod, b->eps, P(T1), P(X1), P(XM2),
             P(MEAN2), P(RSTD2));
  a.up = StArgs{(const bf16_t*)P(XM2), D, (const bf16_t*)P(W_UP_PERM), b->ldw_d, (bf16_t*)u, 2 * F, (bf16_t*)P(H), F, (int)F, nullptr, 0,
                (int)(B * N), (int)(2 * F)};
  a.down.A = (const bf16_t*)P(H);
  a.down.lda = F;
  a.down.W = (const bf16_t*)P(W_DOWN);
  a.down.ldw = b->ldw_f;
  a.down.K = (int)F;
  ch_row_epi(a.down.ep, P(X1), P(GATE2), b->ld_mod, P(NEXT_LN_W), P(NEXT_LN_B), P(NEXT_SCALE), P(NEXT_SHIFT), b->ld_mod, b->next_eps,
             P(T2), P(NEXT_X), P(NEXT_XM), P(NEXT_MEAN), P(NEXT_RSTD));

  constexpr int LDS = ch_lds_bytes();
  static_assert(LDS <= 160 * 1024, "the chain kernel's LDS is the largest phase's");
  static DevOnce once;
  const int n_cu = dev_cus(once, [] {
    (void)hipFuncSetAttribute((const void*)dit_block_fwd_chain_k, hipFuncAttributeMaxDynamicSharedMemorySize, LDS);
  });
  const DlWgCapScope cap_scope(b->max_workgroups);
  // one workgroup per sample up to the workgroup budget; max_workgroups below that is taken as it stands (the budget itself never
  // goes below 8): the workgroups then carry several samples in turn
  const int budget = dl_wg_budget(n_cu);
  int grid = (int)(B < budget ? B : budget);
  if (b->max_workgroups > 0 && b->max_workgroups < grid) grid = b->max_workgroups;
  hipLaunchKernelGGL(dit_block_fwd_chain_k, grid, CH_THREADS, LDS, (hipStream_t)stream, a);
  DL_LAUNCH_CHECK();
  return DL_OK;
}
