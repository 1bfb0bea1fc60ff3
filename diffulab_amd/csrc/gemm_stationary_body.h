// Device body of the activation-stationary NT GEMMs (gemm_stationary.hip has the description, the launchers and the entry points).
// st_gemm_body walks the 256-row panels first, first + stride, ... (count of them) on the calling 512-thread workgroup, with the
// dynamic-LDS base and thread index (threadIdx.x) it is given: gemm_nt_stationary_k calls it with its block index and grid size, the per-sample chain kernel
// (block_fused.hip) with one sample at a time.
#ifndef DIFFULAB_GEMM_STATIONARY_BODY_H
#define DIFFULAB_GEMM_STATIONARY_BODY_H

#include <type_traits>

#include "common.h"

#define ST_THREADS 512
#define ST_PANEL 256  // activation rows per workgroup panel: 8 waves x 32
#define ST_ROWS 64    // weight rows per ring stage: two 32-column MFMA blocks

typedef __attribute__((address_space(3))) void st_lds_void_t;
typedef const __attribute__((address_space(1))) void st_glb_void_t;

struct StArgs {
  const bf16_t* X;
  int64_t ldx;
  const bf16_t* W;
  int64_t ldw;
  bf16_t* C;  // SwiGLU: u = [x1 | x3] or NULL; ssq: the product
  int64_t ldc;
  bf16_t* H;  // SwiGLU only
  int64_t ldh;
  int F;
  float* ssq;  // ssq only
  int ssq_tiles;
  int M, N;
};

// bytes of dynamic LDS of st_gemm_body<NKS, *>: the NST-slot weight ring
template <int NKS>
constexpr int st_lds_bytes() {
  constexpr int STAGE = ST_ROWS * NKS * 128;
  return ((3 * STAGE <= 160 * 1024) ? 3 : 2) * STAGE;
}

template <int N>
__device__ __forceinline__ void st_wait_vmcnt() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// The weight fragments are read with inline assembly and waited for with explicit counted lgkmcnt waits: with compiler-visible reads
// the waitcnt pass put a full lgkmcnt(0) in front of every third MFMA of the read-ahead ring, which exposes the latency of the read
// issued just before it.  LDS reads return in order, so "at most N outstanding" means every read but the N youngest has landed; the
// wait names the register it releases, so that no MFMA on it can be scheduled above the wait.
template <int OFF>
__device__ __forceinline__ void st_lds_read(bf16x8_t& v, unsigned addr) {
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF));
}
template <int N>
__device__ __forceinline__ void st_lds_landed(bf16x8_t& v) {
  asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(v) : "n"(N));
}

static __device__ __forceinline__ void st_lds_landed_n(int n, bf16x8_t& v) {  // (n is a constant once the caller's loop is unrolled)
  if (n >= 3) st_lds_landed<3>(v);
  else if (n == 2) st_lds_landed<2>(v);
  else if (n == 1) st_lds_landed<1>(v);
  else st_lds_landed<0>(v);
}

// EPI 0: fused SwiGLU (N = 2F rows of the permuted weight shadow); EPI 1: plain bf16 store + row sums of squares
template <int NKS, int EPI>
__device__ __forceinline__ void st_gemm_body(const StArgs& a, char* smem, int tid, int first, int stride, int cnt) {
  constexpr int NF = NKS * 4;                                // 16-deep activation fragments per lane
  constexpr int PITCH = NKS * 128;                           // bytes of a weight row in LDS
  constexpr int STAGE = ST_ROWS * PITCH;                     // bytes per ring slot
  constexpr int NST = (3 * STAGE <= 160 * 1024) ? 3 : 2;     // K <= 384: three slots (144 KiB at K = 384)
  constexpr bool WIDE = (PITCH % 256) == 0;                  // which swizzle (see gemm_stationary.hip)
  constexpr int PD = NKS == 8 ? 2 : 3;                       // weight fragments read ahead of their MFMA (K = 512: registers)
  const int lane = tid & 63, hi = lane >> 5, l31 = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int S = a.N / ST_ROWS;                             // stages per panel (even: N % 128 == 0)
  const int total = cnt * S;

  // ---- DMA: wave w copies the 1 KiB chunks w * NKS .. w * NKS + NKS - 1 of a stage; LDS byte o of the stage image holds the 16-byte
  //      slot ((o % PITCH) / 16) ^ g(row) of weight row o / PITCH
  int src_off[NKS];
#pragma unroll
  for (int i = 0; i < NKS; ++i) {
    const int o = (wave * NKS + i) * 1024 + lane * 16;
    const int row = o / PITCH, sl = (o % PITCH) >> 4;
    const int g = WIDE ? (row & 15) : ((row >> 1) & 7);
    src_off[i] = row * (int)a.ldw + ((sl ^ g) << 3);
  }
  int s_it = 0, s_st = 0;  // DMA cursor: stage counter of the workgroup, stage index inside the weight
  auto stage_next = [&]() {
    char* base = smem + (s_it % NST) * STAGE + wave * (NKS * 1024);
    const bf16_t* w = a.W + (int64_t)s_st * ST_ROWS * a.ldw;
#pragma unroll
    for (int i = 0; i < NKS; ++i)
      __builtin_amdgcn_global_load_lds((st_glb_void_t*)(w + src_off[i]), (st_lds_void_t*)(base + i * 1024), 16, 0, 0);
    ++s_it;
    if (++s_st == S) s_st = 0;
  };
  // ---- fragment reads: block b of a stage = weight rows 32b .. 32b+31, lane -> row 32b + l31, k = 16f + 8hi .. + 7
  const int g_rd = WIDE ? (l31 & 15) : ((l31 >> 1) & 7);
  const int rd_base = l31 * PITCH, rd_x = (hi ^ g_rd) << 4;
  const unsigned smem_lds = (unsigned)(uintptr_t)(st_lds_void_t*)smem;

  // acc[2 * h], acc[2 * h + 1]: the two 32-column blocks of a stage; stages alternate between h = 0 and h = 1, so that the blocks of
  // one stage can be stored while the next stage accumulates
  f32x16_t acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
  bf16x8_t x[NF];
  // Waves w and w + 4 share a SIMD and meet at the barrier of every stage.  Were both to run their epilogue arithmetic (the SwiGLU:
  // ~10 VALU instructions per element) at the same point of the stage, the matrix pipe would idle for both epilogues.  The lower four
  // waves therefore store a stage's blocks right behind its MFMAs, the upper four at the start of the NEXT stage, in front of its
  // MFMAs: on every SIMD one wave's epilogue runs under the other wave's MFMAs.  Per wave the epilogues follow one another in stage
  // order either way (the order of the row statistics' additions does not depend on the wave or on the grid).
  const bool upper = wave >= 4;
  int m = 0;        // the row this lane holds as B-operand column and stores
  float ss = 0.f;     // EPI 1: this lane's share of the row's sum of squares inside the current 192-column half of a statistics tile
  float ss_lo = 0.f;  // ... and the row's finished sum over the first half of the tile

#pragma unroll
  for (int s = 0; s < NST - 1; ++s)
    if (s < total) stage_next();

  // ---- epilogue of stage st of the panel (columns 64 st .. 64 st + 63) straight from registers: acc[2h + j][r] = C[m][n] with
  //      n = 64 st + 32 j + 8 (r >> 2) + 4 hi + (r & 3); one v_permlane32_swap per register pair widens a lane's 4 columns to 8
  auto epilogue = [&](auto half_tag, int st) {
    constexpr int HALF = decltype(half_tag)::value;
    const int n_base = st * ST_ROWS;
    if constexpr (EPI == 0) {
      // nt_epilogue_regs<.., 2> (gemm.hip): a 32-column block of the permuted weight is x1 of 16 hidden units, then x3 of the same
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        f32x16_t& c = acc[2 * HALF + j];
        const int u0 = ((n_base + j * 32) >> 1) + 8 * hi;
        float v1[8], v3[8], hv[8], h8[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) hv[e] = silu_f(c[e]) * c[8 + e];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          auto s1 = __builtin_amdgcn_permlane32_swap(__float_as_uint(c[e]), __float_as_uint(c[4 + e]), false, false);
          auto s3 = __builtin_amdgcn_permlane32_swap(__float_as_uint(c[8 + e]), __float_as_uint(c[12 + e]), false, false);
          auto sh = __builtin_amdgcn_permlane32_swap(__float_as_uint(hv[e]), __float_as_uint(hv[4 + e]), false, false);
          v1[e] = __uint_as_float(s1[0]);
          v1[4 + e] = __uint_as_float(s1[1]);
          v3[e] = __uint_as_float(s3[0]);
          v3[4 + e] = __uint_as_float(s3[1]);
          h8[e] = __uint_as_float(sh[0]);
          h8[4 + e] = __uint_as_float(sh[1]);
        }
#pragma unroll
        for (int e = 0; e < 16; ++e) c[e] = 0.f;
        if (a.C) {
          *(u32x4_t*)(a.C + (int64_t)m * a.ldc + u0) = pack8(v1);
          *(u32x4_t*)(a.C + (int64_t)m * a.ldc + a.F + u0) = pack8(v3);
        }
        *(u32x4_t*)(a.H + (int64_t)m * a.ldh + u0) = pack8(h8);
      }
    } else {
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int gp = 0; gp < 2; ++gp) {
          f32x16_t& c = acc[2 * HALF + j];
          float v[8];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            auto sw2 = __builtin_amdgcn_permlane32_swap(__float_as_uint(c[8 * gp + e]), __float_as_uint(c[8 * gp + 4 + e]), false, false);
            v[e] = __uint_as_float(sw2[0]);
            v[4 + e] = __uint_as_float(sw2[1]);
            c[8 * gp + e] = 0.f;
            c[8 * gp + 4 + e] = 0.f;
          }
          const u32x4_t pk = pack8(v);
          *(u32x4_t*)(a.C + (int64_t)m * a.ldc + n_base + j * 32 + 16 * gp + 8 * hi) = pk;
          float r[8];
          unpack8(pk, r);
#pragma unroll
          for (int e = 0; e < 8; ++e) ss += r[e] * r[e];
        }
      // A 384-wide statistics tile is six stages (the last tile of the row may be narrower).  The grouping of nt_epilogue_ssq is kept:
      // there a wave sums 192 columns of the row -- per lane in this very order, then the two lane halves (xor32_sum) -- and the
      // tile's two column waves meet as two addends on a zeroed word, so the sum below has its bits.
      if (st % 6 == 2) {
        ss_lo = xor32_sum(ss);
        ss = 0.f;
      }
      if ((st + 1) % 6 == 0 || st + 1 == S) {
        if (st / 6 < a.ssq_tiles) {
          const float t = ss_lo + xor32_sum(ss);
          if (hi == 0) a.ssq[(int64_t)m * a.ssq_tiles + st / 6] = t;
        }
        ss = 0.f;
        ss_lo = 0.f;
      }
    }
  };

  int it = 0;
  // stage st of the panel: weight rows 64 st .. 64 st + 63, accumulated in acc[2 * HALF], acc[2 * HALF + 1]
  auto stage = [&](auto half_tag, int st) {
    constexpr int HALF = decltype(half_tag)::value;
    // Stage `it` must have landed.  Per wave the vector-memory counter is in issue order: behind the DMA of stage `it` sit the DMAs of
    // the NST-2 younger stages and the stores of at least one epilogue (lower waves, three slots: of two -- the wait is then stricter
    // than needed, the older one's stores have to land as well; likewise when a statistics store follows an epilogue's).  In the first
    // two stages of a panel everything older was drained at the panel start and fewer stores may have been issued since: no stores
    // are assumed behind the DMA.  At the end of the stream no younger DMA exists: drain.
    constexpr int YOUNG = (NST - 2) * NKS;
    if (it + NST - 2 < total) {
      if (st < 2) st_wait_vmcnt<YOUNG>();
      else if (EPI == 1) st_wait_vmcnt<YOUNG + 4>();
      else if (a.C) st_wait_vmcnt<YOUNG + 6>();
      else st_wait_vmcnt<YOUNG + 2>();
    } else {
      st_wait_vmcnt<0>();
    }
    __builtin_amdgcn_s_barrier();  // raw: every wave's share of stage `it` has landed, and every wave is done with stage it-1
    if (NST < 3 && s_it < total) stage_next();  // into the slot of stage it-1
    if (upper && st > 0) epilogue(std::integral_constant<int, 1 - HALF>{}, st - 1);
    const unsigned sw = smem_lds + (it % NST) * STAGE + rd_base;
    bf16x8_t wq[PD + 1];
    // byte (f << 5) ^ rd_x of the row: the XOR touches bits 4..7 only, so fragments f and f + 8 differ by the constant 256 -- eight
    // per-lane addresses serve every fragment, the rest is the instruction's immediate offset
    auto rd = [&](int s) {  // s = 2 * fragment + block
      const int f = s >> 1;
      const unsigned ad = sw + (((f & 7) << 5) ^ rd_x);
      bf16x8_t& v = wq[s % (PD + 1)];
      switch ((f >> 3) * 2 + (s & 1)) {  // (a constant once the loop is unrolled)
        case 0: st_lds_read<0>(v, ad); break;
        case 1: st_lds_read<32 * PITCH>(v, ad); break;
        case 2: st_lds_read<256>(v, ad); break;
        case 3: st_lds_read<32 * PITCH + 256>(v, ad); break;
        case 4: st_lds_read<512>(v, ad); break;
        case 5: st_lds_read<32 * PITCH + 512>(v, ad); break;
        case 6: st_lds_read<768>(v, ad); break;
        default: st_lds_read<32 * PITCH + 768>(v, ad); break;
      }
    };
#pragma unroll
    for (int s = 0; s < PD; ++s) rd(s);
#pragma unroll
    for (int s = 0; s < 2 * NF; ++s) {
      __builtin_amdgcn_sched_barrier(0);
      if (s + PD < 2 * NF) rd(s + PD);
      st_lds_landed_n(2 * NF - 1 - s < PD ? 2 * NF - 1 - s : PD, wq[s % (PD + 1)]);  // reads return in order: fragment s has landed
      acc[2 * HALF + (s & 1)] =
          __builtin_amdgcn_mfma_f32_32x32x16_bf16(wq[s % (PD + 1)], x[s >> 1], acc[2 * HALF + (s & 1)], 0, 0, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
    if (NST >= 3 && s_it < total) stage_next();  // into the slot of stage it-1
    if (!upper) epilogue(half_tag, st);
    ++it;
  };

  int panel = first;
  for (int p = 0; p < cnt; ++p, panel += stride) {
    m = panel * ST_PANEL + wave * 32 + l31;
    {
      const bf16_t* xr = a.X + (int64_t)m * a.ldx + hi * 8;
#pragma unroll
      for (int f = 0; f < NF; ++f) x[f] = *(const bf16x8_t*)(xr + f * 16);
      st_wait_vmcnt<0>();  // the panel, and with it everything older: the waits in stage() count from here
#pragma unroll
      for (int f = 0; f < NF; ++f) asm volatile("" : "+v"(x[f]));  // (the compiler's own wait for these loads stays here too)
    }
    for (int st = 0; st < S; st += 2) {
      stage(std::integral_constant<int, 0>{}, st);
      stage(std::integral_constant<int, 1>{}, st + 1);
    }
    if (upper) epilogue(std::integral_constant<int, 1>{}, S - 1);
  }
}

#endif  // DIFFULAB_GEMM_STATIONARY_BODY_H
