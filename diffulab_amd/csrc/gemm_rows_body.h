// Device body of the row-complete GEMMs (gemm_ln.hip has the description, the launchers and the entry points).  rk_gemm_body walks
// the 256 x 384 tiles first, first + stride, ... (count of them) on the calling 512-thread workgroup, with the dynamic-LDS base and thread
// index (threadIdx.x) it is given: gemm_nt_rows_k calls it with its slot of the grid, the per-sample chain kernel (block_fused.hip) with one sample at a time.
#ifndef DIFFULAB_GEMM_ROWS_BODY_H
#define DIFFULAB_GEMM_ROWS_BODY_H

#include "common.h"

typedef __attribute__((address_space(3))) void lds_void_t;
typedef const __attribute__((address_space(1))) void glb_void_t;

// Direct-to-LDS 16-byte load in the SGPR-base + 32-bit lane-offset form.  Inline assembly on purpose: through the builtin the
// compiler materialises a 64-bit per-lane address for every chunk (20 VGPRs that it then spills next to the 192 accumulators,
// and a scratch reload inside the k-loop waits on vmcnt(0), i.e. drains the operand ring).  M0 (the LDS destination base) is
// compiler-reserved: it is saved and restored inside the statement.  The statement is not part of the compiler's vmcnt
// bookkeeping; every wait for these loads in this file is an explicit rk_wait_vmcnt.
static __device__ __forceinline__ void glds16_s(const void* sbase, uint32_t voff, const void* lds_dst_wave_base) {
  uint32_t keep;
  const uint32_t dst = (uint32_t)(uintptr_t)(lds_void_t*)lds_dst_wave_base;
  asm volatile("s_nop 4\n\ts_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
               : "=&s"(keep)
               : "v"(voff), "s"(sbase), "s"(dst)
               : "memory");
}

#define RK_BM 256
#define RK_BN 384
#define RK_BK 64
#define RK_THREADS 512
#define RK_STAGE ((RK_BM + RK_BN) * 128)  // bytes per ring slot (81920)
#define RK_CH 10                          // 1 KiB DMA chunks per wave per stage
#define RK_JN 6                           // 32-wide MFMA column tiles per wave
#define RK_PITCH 784                      // bytes per row of the epilogue's LDS piece
#define RK_D8 48                          // 16-byte chunks per 384-wide row = active lanes of a row wave

enum { RK_LNF = 0, RK_LNB = 1, RK_QK = 2 };

struct RowEpi {
  // ---- RK_LNF
  const bf16_t* resid;   // [M, D] residual stream before the gated add, or NULL (x = t: patch embedding)
  const bf16_t* gate;    // row view [groups, ld_gate] or NULL (then x = resid + t)
  int64_t ld_gate;
  const float* ln_w;     // f32 [D] or NULL (no affine)
  const float* ln_b;
  const bf16_t* scale;   // row views [groups, ld_mod]
  const bf16_t* shift;
  int64_t ld_mod;
  float eps;
  bf16_t* t_out;         // [M, D] GEMM result as bf16 (NULL: not kept)
  bf16_t* x_out;         // [M, D] new residual stream (NULL: not kept -- only legal when resid == NULL and nobody reads it)
  bf16_t* xm_out;        // [M, D] modulated rows
  float* mean;           // f32 [M]
  float* rstd;
  // ---- RK_LNB (ln_w, ln_b, scale, ld_mod, gate, ld_gate as above; gate = the gate of the residual that follows in the chain)
  const bf16_t* x;       // [M, D] LayerNorm input of the forward
  const float* mean_i;   // f32 [M]
  const float* rstd_i;
  const bf16_t* dres;    // [M, D] or NULL
  bf16_t* dx;            // [M, D]
  float* dscale;         // f32 row views [groups, ld_dmod], written (=)
  float* dshift;
  int64_t ld_dmod;
  float* dwb;            // f32 [groups, 2, D] written (=), or NULL
  const bf16_t* gt;      // [M, D] t of the gated residual that follows, or NULL
  bf16_t* gdt;           // [M, D]
  float* dgate;          // f32 row view, written (=)
  // ---- RK_QK
  bf16_t* qkv;           // [M, 3D] pre-norm rows
  bf16_t* qo;            // [B, H, n_dst, dh]
  bf16_t* ko;
  float* rrms;           // f32 [M, 2]
  const float* sq;       // f32 [D]
  const float* sk;
  const float* cs;       // f32 [tokens, rot/2]
  const float* sn;
  int n_tok, heads, dh, rot, n_dst, n_off;
};

template <int N>
static __device__ __forceinline__ void rk_wait_vmcnt() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
static __device__ __forceinline__ void rk_lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

static __device__ __forceinline__ u32x4_t rk_ld16(const bf16_t* p) { return *(const u32x4_t*)p; }

// ---------------------------------------------------------------------------------------------------------------------
// epilogue: P[j][i][q] = bf16 pairs of acc[j][i][2q], acc[j][i][2q+1]  (tile row wm*64 + i*32 + (lane & 31),
// tile column wn*192 + j*32 + 8*(r >> 2) + 4*hi + (r & 3), r = accumulator register)
// ---------------------------------------------------------------------------------------------------------------------
template <int MODE>
static __device__ __forceinline__ void rk_row_epilogue(uint32_t (&P)[RK_JN][2][8], char* lds, int tile_m, int tile_n, int lane,
                                                       int wave, const RowEpi& ep) {
  constexpr int D = RK_BN;
  const int hi = lane >> 5, wm = wave >> 1, wn = wave & 1;
  const bool on = lane < RK_D8;
  const int64_t m0 = (int64_t)tile_m * RK_BM;
  const int64_t g = tile_m;  // modulation group = sample (256 rows per group)
  const float invD = 1.0f / (float)D;
  const int c8 = lane * 8;   // first column of this lane's chunk (row waves)

  // ---- per-tile constants of the row loop (lane = column chunk)
  float k0[8], k1[8], k2[8], k3[8], k4[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) k0[e] = k1[e] = k2[e] = k3[e] = k4[e] = 0.f;
  if constexpr (MODE == RK_LNF) {
    // k0 = w, k1 = b, k2 = scale, k3 = shift, k4 = gate
    if (on) {
      if (ep.ln_w) {
        *(f32x4_t*)&k0[0] = *(const f32x4_t*)(ep.ln_w + c8);
        *(f32x4_t*)&k0[4] = *(const f32x4_t*)(ep.ln_w + c8 + 4);
        *(f32x4_t*)&k1[0] = *(const f32x4_t*)(ep.ln_b + c8);
        *(f32x4_t*)&k1[4] = *(const f32x4_t*)(ep.ln_b + c8 + 4);
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) k0[e] = 1.0f;
      }
      unpack8(rk_ld16(ep.scale + g * ep.ld_mod + c8), k2);
      unpack8(rk_ld16(ep.shift + g * ep.ld_mod + c8), k3);
      if (ep.gate) unpack8(rk_ld16(ep.gate + g * ep.ld_gate + c8), k4);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) k0[e] = 1.0f;
    }
  } else if constexpr (MODE == RK_LNB) {
    // k0 = (1 + scale) * w, k4 = gate of the residual that follows; k1..k3 = the three column accumulators S1, S2, S3
    if (on) {
      float wv[8], sc[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) wv[e] = 1.0f;
      if (ep.ln_w) {
        *(f32x4_t*)&wv[0] = *(const f32x4_t*)(ep.ln_w + c8);
        *(f32x4_t*)&wv[4] = *(const f32x4_t*)(ep.ln_w + c8 + 4);
      }
      unpack8(rk_ld16(ep.scale + g * ep.ld_mod + c8), sc);
#pragma unroll
      for (int e = 0; e < 8; ++e) k0[e] = (1.0f + sc[e]) * wv[e];
      if (ep.gt) unpack8(rk_ld16(ep.gate + g * ep.ld_gate + c8), k4);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) k0[e] = 1.0f;
    }
  } else {
    // k0 = RMSNorm scale of this tile's third (q or k)
    if (on && tile_n < 2) {
      const float* s = tile_n == 0 ? ep.sq : ep.sk;
      *(f32x4_t*)&k0[0] = *(const f32x4_t*)(s + c8);
      *(f32x4_t*)&k0[4] = *(const f32x4_t*)(s + c8 + 4);
    }
  }

  // ---- global operands of a row, fetched one row ahead of its use
  u32x4_t pa = {0, 0, 0, 0}, pb = {0, 0, 0, 0}, pc = {0, 0, 0, 0};
  float pf0 = 0.f, pf1 = 0.f;
  auto row_of = [&](int s) -> int64_t {  // s = (i * 2 + pair) * 8 + rr: the s-th row this wave processes
    const int i = s >> 4, pair = (s >> 3) & 1, lr = (s & 7) * 8 + wave;
    return m0 + (2 * pair + (lr >> 5)) * 64 + i * 32 + (lr & 31);
  };
  auto fetch = [&](int s) {
    const int64_t row = row_of(s);
    if constexpr (MODE == RK_LNF) {
      if (on && ep.resid) pa = rk_ld16(ep.resid + row * D + c8);
    } else if constexpr (MODE == RK_LNB) {
      if (on) {
        pa = rk_ld16(ep.x + row * D + c8);
        if (ep.dres) pb = rk_ld16(ep.dres + row * D + c8);
        if (ep.gt) pc = rk_ld16(ep.gt + row * D + c8);
      }
      pf0 = ep.mean_i[row];
      pf1 = ep.rstd_i[row];
    } else {
      if (on && tile_n < 2) {
        const int dh = ep.dh, h = c8 / dh, d0 = c8 - h * dh;
        if (d0 < ep.rot) {
          const int n = (int)(row % ep.n_tok);
          const f32x4_t cc = *(const f32x4_t*)(ep.cs + (int64_t)n * (ep.rot >> 1) + (d0 >> 1));
          const f32x4_t ss = *(const f32x4_t*)(ep.sn + (int64_t)n * (ep.rot >> 1) + (d0 >> 1));
          pa = __builtin_bit_cast(u32x4_t, cc);
          pb = __builtin_bit_cast(u32x4_t, ss);
        }
      }
    }
  };

  fetch(0);
  rk_lds_barrier();  // every wave has finished the fragment reads of the last k-step: its ring slot is free
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    for (int pair = 0; pair < 2; ++pair) {
      // ---- dump 64 rows (this i of the waves wm = 2 pair, 2 pair + 1) as bf16: 16-byte chunks of 8 consecutive columns
      if ((wm >> 1) == pair) {
        char* base = lds + ((wm & 1) * 32 + (lane & 31)) * RK_PITCH + (wn * 192 + 8 * hi) * 2;
#pragma unroll
        for (int j = 0; j < RK_JN; ++j)
#pragma unroll
          for (int gp = 0; gp < 2; ++gp) {
            const auto s0 = __builtin_amdgcn_permlane32_swap(P[j][i][4 * gp + 0], P[j][i][4 * gp + 2], false, false);
            const auto s1 = __builtin_amdgcn_permlane32_swap(P[j][i][4 * gp + 1], P[j][i][4 * gp + 3], false, false);
            u32x4_t v = {s0[0], s1[0], s0[1], s1[1]};
            *(u32x4_t*)(base + (j * 32 + 16 * gp) * 2) = v;
          }
      }
      rk_lds_barrier();
      for (int rr = 0; rr < 8; ++rr) {
        const int s = (i * 2 + pair) * 8 + rr;
        const int lr = rr * 8 + wave;
        const int64_t row = row_of(s);
        const u32x4_t qa = pa, qb = pb, qc = pc;
        const float f0 = pf0, f1 = pf1;
        if (s + 1 < 32) fetch(s + 1);
        u32x4_t tq = {0, 0, 0, 0};
        if (on) tq = *(const u32x4_t*)(lds + lr * RK_PITCH + lane * 16);
        float tv[8];
        unpack8(tq, tv);

        if constexpr (MODE == RK_LNF) {
          if (on && ep.t_out) *(u32x4_t*)(ep.t_out + row * D + c8) = tq;
          float xv[8];
          if (ep.resid) {
            unpack8(qa, xv);
            if (ep.gate) {
#pragma unroll
              for (int e = 0; e < 8; ++e) xv[e] = bf2f(f2bf(xv[e] + k4[e] * tv[e]));  // statistics of what is stored
            } else {
#pragma unroll
              for (int e = 0; e < 8; ++e) xv[e] = bf2f(f2bf(xv[e] + tv[e]));
            }
          } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) xv[e] = tv[e];
          }
          if (on && ep.x_out) *(u32x4_t*)(ep.x_out + row * D + c8) = pack8(xv);
          float sm = 0.f;
#pragma unroll
          for (int e = 0; e < 8; ++e) sm += xv[e];
          const float mu = wave_sum(sm) * invD;
          float q = 0.f;
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float d = on ? (xv[e] - mu) : 0.f;
            q += d * d;
          }
          const float rs = rsqrtf(wave_sum(q) * invD + ep.eps);
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float y = (xv[e] - mu) * rs * k0[e] + k1[e];
            xv[e] = y * (1.0f + k2[e]) + k3[e];
          }
          if (on) *(u32x4_t*)(ep.xm_out + row * D + c8) = pack8(xv);
          if (lane == 0) {
            ep.mean[row] = mu;
            ep.rstd[row] = rs;
          }
        } else if constexpr (MODE == RK_LNB) {
          float xv[8], rv[8];
          unpack8(qa, xv);
#pragma unroll
          for (int e = 0; e < 8; ++e) rv[e] = 0.f;
          if (ep.dres) unpack8(qb, rv);
          const float mu = f0, rs = f1;
          float s1 = 0.f, s2 = 0.f;
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float xh = on ? (xv[e] - mu) * rs : 0.f;
            const float d = tv[e];
            k1[e] += d;
            k2[e] += d * xh;
            const float dxh = d * k0[e];
            s1 += dxh;
            s2 += dxh * xh;
            xv[e] = xh;
            tv[e] = dxh;
          }
          const float c1 = wave_sum(s1) * invD, c2 = wave_sum(s2) * invD;
#pragma unroll
          for (int e = 0; e < 8; ++e) rv[e] += rs * (tv[e] - c1 - xv[e] * c2);
          if (on) *(u32x4_t*)(ep.dx + row * D + c8) = pack8(rv);
          if (ep.gt) {
            float gtv[8];
            unpack8(qc, gtv);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              const float dxr = bf2f(f2bf(rv[e]));
              k3[e] += on ? dxr * gtv[e] : 0.f;
              rv[e] = dxr * k4[e];
            }
            if (on) *(u32x4_t*)(ep.gdt + row * D + c8) = pack8(rv);
          }
        } else {
          // pre-norm row of this third of qkv (the backward's input; V is read in place by the attention kernels)
          if (on) *(u32x4_t*)(ep.qkv + row * (3 * D) + tile_n * D + c8) = tq;
          if (tile_n < 2) {
            float s1 = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) s1 += tv[e] * tv[e];
            const float rq = rsqrtf(wave_sum(s1) * invD + ep.eps);
            if (on) {
              const int dh = ep.dh, h = c8 / dh, d0 = c8 - h * dh;
#pragma unroll
              for (int e = 0; e < 8; ++e) tv[e] = tv[e] * rq * k0[e];
              if (d0 < ep.rot) {
                const f32x4_t cc = __builtin_bit_cast(f32x4_t, qa), ss = __builtin_bit_cast(f32x4_t, qb);
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                  const float a = tv[2 * p], b = tv[2 * p + 1];
                  tv[2 * p] = a * cc[p] - b * ss[p];
                  tv[2 * p + 1] = a * ss[p] + b * cc[p];
                }
              }
              const int64_t bb = row / ep.n_tok;
              const int n = (int)(row - bb * ep.n_tok);
              const int64_t o = ((bb * ep.heads + h) * ep.n_dst + ep.n_off + n) * dh + d0;
              *(u32x4_t*)((tile_n == 0 ? ep.qo : ep.ko) + o) = pack8(tv);
            }
            if (lane == 0) ep.rrms[row * 2 + tile_n] = rq;
          }
        }
      }
      rk_lds_barrier();  // the piece is rewritten by the next dump (or by the next tile's operand DMA)
    }
  }

  if constexpr (MODE == RK_LNB) {
    // ---- per-sample column sums: one [3][D] f32 slot per wave, summed in wave order (deterministic), plain stores
    float* red = (float*)lds;
    if (on) {
      float* slot = red + (size_t)wave * 3 * D + c8;
      *(f32x4_t*)(slot) = *(f32x4_t*)&k1[0];
      *(f32x4_t*)(slot + 4) = *(f32x4_t*)&k1[4];
      *(f32x4_t*)(slot + D) = *(f32x4_t*)&k2[0];
      *(f32x4_t*)(slot + D + 4) = *(f32x4_t*)&k2[4];
      *(f32x4_t*)(slot + 2 * D) = *(f32x4_t*)&k3[0];
      *(f32x4_t*)(slot + 2 * D + 4) = *(f32x4_t*)&k3[4];
    }
    rk_lds_barrier();
    const int col = threadIdx.x;
    if (col < D) {
      float S1 = 0.f, S2 = 0.f, S3 = 0.f;
#pragma unroll
      for (int w = 0; w < 8; ++w) {
        S1 += red[(size_t)w * 3 * D + col];
        S2 += red[(size_t)w * 3 * D + D + col];
        S3 += red[(size_t)w * 3 * D + 2 * D + col];
      }
      const float wc = ep.ln_w ? ep.ln_w[col] : 1.0f, bc = ep.ln_b ? ep.ln_b[col] : 0.0f;
      const float sc1 = 1.0f + bf2f(ep.scale[g * ep.ld_mod + col]);
      ep.dscale[g * ep.ld_dmod + col] = wc * S2 + bc * S1;
      ep.dshift[g * ep.ld_dmod + col] = S1;
      if (ep.gt) ep.dgate[g * ep.ld_dmod + col] = S3;
      if (ep.dwb) {
        ep.dwb[(size_t)g * 2 * D + col] = sc1 * S2;
        ep.dwb[(size_t)g * 2 * D + D + col] = sc1 * S1;
      }
    }
    rk_lds_barrier();
  }
}

// tiles first, first + stride, ... (cnt of them; tile = panel * (N / 384) + column tile) of C = A . Bm^T, each followed by its row
// epilogue.  smem: 2 * RK_STAGE bytes of dynamic LDS.
template <int MODE>
static __device__ __forceinline__ void rk_gemm_body(const bf16_t* __restrict__ A, int64_t lda, const bf16_t* __restrict__ Bm,
                                                    int64_t ldb, int N, int K, const RowEpi& ep, char* smem, int tid, int first,
                                                    int stride, int cnt) {
  const int lane = tid & 63, hi = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int tiles_n = N / RK_BN;
  const int nk = K / RK_BK;
  const int total = cnt * nk;

  // DMA cursor: one stage ahead of the compute cursor
  int s_tile = first, s_kt = 0, s_it = 0;
  const bf16_t* s_ta = A + (int64_t)((s_tile / tiles_n) * RK_BM) * lda;
  const bf16_t* s_tb = Bm + (int64_t)((s_tile % tiles_n) * RK_BN) * ldb;

  f32x16_t acc[RK_JN][2];
#pragma unroll
  for (int j = 0; j < RK_JN; ++j)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[j][i][r] = 0.f;

  int it = 0;
  for (int t = 0; t < cnt; ++t) {
    const int tile = first + t * stride;
    // Per-lane constants of the main loop are re-derived for every tile from an opaque copy of the lane id: kept live across
    // the row epilogue they were spilled, and a scratch reload in the k-loop waits on vmcnt(0), i.e. drains the operand DMA.
    int ln = lane;
    asm volatile("" : "+v"(ln));
    const int lhi = ln >> 5;
    uint32_t src_off[RK_CH];  // byte offset of this lane's 16 bytes inside the A / B row panel of a tile (k = 0)
    int lds_off[RK_CH];
    bool is_a[RK_CH];
#pragma unroll
    for (int i = 0; i < RK_CH; ++i) {
      const int c = wave * RK_CH + i;
      is_a[i] = c < RK_BM / 8;
      const int cc = is_a[i] ? c : c - RK_BM / 8;
      const int r = cc * 8 + (ln >> 3);
      const int q = (ln & 7) ^ ((r >> 1) & 7);
      src_off[i] = (uint32_t)(r * (int)(is_a[i] ? lda : ldb) + q * 8) * 2u;
      lds_off[i] = (is_a[i] ? 0 : RK_BM * 128) + cc * 1024;
    }
    auto stage_next = [&]() {
      char* base = smem + (s_it & 1) * RK_STAGE;
      const char* ka = (const char*)(s_ta + s_kt * RK_BK);
      const char* kb = (const char*)(s_tb + s_kt * RK_BK);
#pragma unroll
      for (int i = 0; i < RK_CH; ++i) glds16_s(is_a[i] ? ka : kb, src_off[i], base + lds_off[i]);
      ++s_it;
      if (++s_kt == nk) {
        s_kt = 0;
        s_tile += stride;
        s_ta = A + (int64_t)((s_tile / tiles_n) * RK_BM) * lda;
        s_tb = Bm + (int64_t)((s_tile % tiles_n) * RK_BN) * ldb;
      }
    };
    int xrow[2], wrow[RK_JN];
#pragma unroll
    for (int i = 0; i < 2; ++i) xrow[i] = wm * 64 + i * 32 + (ln & 31);
#pragma unroll
    for (int j = 0; j < RK_JN; ++j) wrow[j] = wn * (RK_BN / 2) + j * 32 + (ln & 31);

    if (t == 0) stage_next();
    for (int kt = 0; kt < nk; ++kt, ++it) {
      rk_wait_vmcnt<0>();             // stage `it` has landed (two-slot ring: nothing younger is in flight)
      __builtin_amdgcn_s_barrier();   // raw barrier: every wave's DMA share has landed and the other slot's readers are done
      if (s_it < total) stage_next();
      const char* sa = smem + (it & 1) * RK_STAGE;
      const char* sb = sa + RK_BM * 128;
      // fragment software pipeline of gemm_nt_big_k: weight fragment two MFMA pairs ahead, activation fragments one sub-step ahead
      bf16x8_t xq[2][2], wq[3];
      auto rd_x = [&](int kk, int i) -> bf16x8_t {
        return *(const bf16x8_t*)(sa + xrow[i] * 128 + ((((kk << 1) | lhi) ^ ((xrow[i] >> 1) & 7)) << 4));
      };
      auto rd_w = [&](int kk, int j) -> bf16x8_t {
        return *(const bf16x8_t*)(sb + wrow[j] * 128 + ((((kk << 1) | lhi) ^ ((wrow[j] >> 1) & 7)) << 4));
      };
      xq[0][0] = rd_x(0, 0);
      xq[0][1] = rd_x(0, 1);
      wq[0] = rd_w(0, 0);
      wq[1] = rd_w(0, 1);
#pragma unroll
      for (int s = 0; s < 4 * RK_JN; ++s) {
        const int kk = s / RK_JN, j = s % RK_JN;
        __builtin_amdgcn_sched_barrier(0);
        if (s + 2 < 4 * RK_JN) wq[(s + 2) % 3] = rd_w((s + 2) / RK_JN, (s + 2) % RK_JN);
        if (kk < 3 && j < 2) xq[(kk + 1) & 1][j] = rd_x(kk + 1, j);
#pragma unroll
        for (int i = 0; i < 2; ++i) acc[j][i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wq[s % 3], xq[kk & 1][i], acc[j][i], 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    uint32_t P[RK_JN][2][8];
#pragma unroll
    for (int j = 0; j < RK_JN; ++j)
#pragma unroll
      for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int q = 0; q < 8; ++q) P[j][i][q] = pack2bf(acc[j][i][2 * q], acc[j][i][2 * q + 1]);
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][i][r] = 0.f;
      }
    // the slot consumed by the last k-step; the other one may already be receiving the next tile's first stage
    rk_row_epilogue<MODE>(P, smem + ((it - 1) & 1) * RK_STAGE, tile / tiles_n, tile % tiles_n, lane, wave, ep);
  }
}

#endif  // DIFFULAB_GEMM_ROWS_BODY_H
