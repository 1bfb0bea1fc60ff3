// Tile helpers of the attention kernels (attention.hip has the description) and the device body of the persistent, pipelined forward
// with QK-RMSNorm + RoPE on load.  attn_qkn_pipe_body walks the (sample, head) items first, first + stride, ... (count of them) on the
// calling 512-thread workgroup, with the dynamic-LDS base and thread index (threadIdx.x) it is given: attn_fwd_qkn_pipe_k calls it with its run of items, the
// per-sample chain kernel (block_fused.hip) with the heads of one sample.
#ifndef DIFFULAB_ATTENTION_BODY_H
#define DIFFULAB_ATTENTION_BODY_H

#include "common.h"

typedef __attribute__((address_space(3))) void lds_void_t;
typedef const __attribute__((address_space(1))) void glb_void_t;

#define DH 64
#define ROWB 128  // bytes per LDS tile row (64 bf16)
#define LOG2E 1.4426950408889634f
#define LN2 0.6931471805599453f

// 16-byte-slot swizzle of a [rows][64 bf16] tile: conflict-free for ds_read_b128 by 16 consecutive rows
// (bijection of (row>>1)&7) AND for ds_read_b64_tr_b16 blocks of 4 consecutive rows (bit 2 separates rows r, r+2).
__device__ __forceinline__ int swz8(int row) {
  const int v = (row >> 1) & 7;
  return ((v & 1) << 2) | (v >> 1);
}
__device__ __forceinline__ int tile_off(int row, int slot) { return row * ROWB + ((slot ^ swz8(row)) << 4); }

// DMA rows [0, nrows) of a row-major [nrows][64] bf16 matrix (row pitch `pitch` elements) into an LDS tile.
__device__ __forceinline__ void tile_dma(const bf16_t* __restrict__ g, int64_t pitch, char* tile, int nrows, int wave,
                                         int nwaves, int lane) {
  const int nchunk = nrows >> 3;  // 8 rows = 1 KiB per wave-instruction
  for (int c = wave; c < nchunk; c += nwaves) {
    const int r = c * 8 + (lane >> 3);
    const int q = (lane & 7) ^ swz8(r);
    __builtin_amdgcn_global_load_lds((glb_void_t*)(g + (int64_t)r * pitch + q * 8), (lds_void_t*)(tile + c * 1024), 16, 0, 0);
  }
}

// A/B fragment with k = head-dim: row `row` of the tile, k-slots 16*ks + 8*hi .. +7
__device__ __forceinline__ bf16x8_t frag_rows(const char* tile, int row, int ks, int hi) {
  return *(const bf16x8_t*)(tile + tile_off(row, ks * 2 + hi));
}
// A fragment with k = tile rows (transposing read): output row i = head-dim column colbase + (lane&31),
// k-slot j of half hi <-> tile row rbase + (j&3) + 8*(j>>2) + 4*hi
__device__ __forceinline__ bf16x8_t frag_cols(const char* tile, int rbase, int colbase, int lane) {
  const int li = lane & 15, g = lane >> 4;
  const int col = colbase + (g & 1) * 16 + (li & 3) * 4;
  const int r0 = rbase + (g >> 1) * 4 + (li >> 2);
  union {
    s16x4_t h[2];
    bf16x8_t v;
  } u;
  u.h[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (__attribute__((address_space(3))) s16x4_t*)(tile + r0 * ROWB + (((col >> 3) ^ swz8(r0)) << 4) + (col & 7) * 2));
  const int r1 = r0 + 8;
  u.h[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (__attribute__((address_space(3))) s16x4_t*)(tile + r1 * ROWB + (((col >> 3) ^ swz8(r1)) << 4) + (col & 7) * 2));
  return u.v;
}
// frag_cols' transposing read as inline asm: the compiler sees no LDS read, so puts no wait for an in-flight DMA in front of it
__device__ __forceinline__ s16x4_t attn_lds_tr16(const char* p) {
  s16x4_t v;
  asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(v) : "v"((unsigned)(uintptr_t)(lds_void_t*)p));
  return v;
}
__device__ __forceinline__ bf16x8_t pack_frag(const float* p) {
  union {
    u32x4_t u;
    bf16x8_t v;
  } r;
#pragma unroll
  for (int i = 0; i < 4; ++i) r.u[i] = pack2bf(p[2 * i], p[2 * i + 1]);
  return r.v;
}
// raw v_exp_f32: exp2f() wraps it in a denormal-range rescale (cmp / cndmask / add / ldexp, 6 VALU instructions per element, half of
// the backward kernel's VALU stream); a probability below 2^-126 flushing to zero is exactly what softmax wants
__device__ __forceinline__ float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }
#define MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0)

// store a transposed 64-column accumulator pair (lane & 31 = row, register r <-> column 8*(r>>2) + 4*hi + (r&3) of each 32-wide
// half) as bf16: one v_permlane32_swap per register pair gives every lane 8 consecutive columns = one 16-byte store, 32 contiguous
// bytes per row and instruction (the GEMM epilogue's scheme) instead of 8-byte stores
__device__ __forceinline__ void store_rows64(bf16_t* rowp, const f32x16_t (&a)[2], float mul, int hi) {
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int gp = 0; gp < 2; ++gp) {
      float v[8];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(a[dt][8 * gp + e] * mul), __float_as_uint(a[dt][8 * gp + 4 + e] * mul),
                                                   false, false);
        v[e] = __uint_as_float(sw[0]);
        v[4 + e] = __uint_as_float(sw[1]);
      }
      *(u32x4_t*)(rowp + dt * 32 + 16 * gp + 8 * hi) = pack8(v);
    }
}

// the same packing without the stores: pk[dt * 2 + gp] = the 16 bytes store_rows64 writes at column 32 dt + 16 gp + 8 hi
__device__ __forceinline__ void pack_rows64(u32x4_t (&pk)[4], const f32x16_t (&a)[2], float mul) {
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int gp = 0; gp < 2; ++gp) {
      float v[8];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(a[dt][8 * gp + e] * mul), __float_as_uint(a[dt][8 * gp + 4 + e] * mul),
                                                   false, false);
        v[e] = __uint_as_float(sw[0]);
        v[4 + e] = __uint_as_float(sw[1]);
      }
      pk[dt * 2 + gp] = pack8(v);
    }
}

// ------------------------------------------------------------------------------ QK-RMSNorm + RoPE on load (attention.hip)
struct QkNorm {
  const float* ssq;   // f32 [B*N, 2]: sums of squares of the q / k rows
  const float* sq;    // f32 [D] query_norm.scale
  const float* sk;    // f32 [D] key_norm.scale
  const float* cs;    // f32 [N, rot/2]
  const float* sn;
  bf16_t* qo;         // [B, H, N, 64] normalised + rotated q (kept for the backward)
  bf16_t* ko;
  float* rrms;        // f32 [B*N, 2]
  float inv_d, eps;
  int rot;
  int pitch;          // elements between token rows of qkv (3 D)
};
__device__ __forceinline__ u32x4_t qk_xform8(u32x4_t raw, float r, const float* __restrict__ s8, const float* __restrict__ c4,
                                             const float* __restrict__ n4, bool rotary) {
  float x[8];
  unpack8(raw, x);
  const f32x4_t s0 = *(const f32x4_t*)s8, s1 = *(const f32x4_t*)(s8 + 4);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    x[e] = x[e] * r * s0[e];
    x[4 + e] = x[4 + e] * r * s1[e];
  }
  if (rotary) {
    const f32x4_t cc = *(const f32x4_t*)c4, ss = *(const f32x4_t*)n4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float a = x[2 * i], b = x[2 * i + 1];
      x[2 * i] = a * cc[i] - b * ss[i];
      x[2 * i + 1] = a * ss[i] + b * cc[i];
    }
  }
  return pack8(x);
}

#define PIPE_N 256
// dynamic LDS of attn_qkn_pipe_body: two K / V tile pairs and the QK-norm scales of every head
constexpr int attn_pipe_lds_bytes(int D) { return 4 * PIPE_N * ROWB + 8 * D; }

// the persistent + pipelined forward over the items first, first + stride, ... (count of them; item = sample * H + head)
__device__ __forceinline__ void attn_qkn_pipe_body(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ out, float* __restrict__ lse,
                                                   int H, float scale, const QkNorm& qn, char* smem, int tid, int first, int stride,
                                                   int count) {
  constexpr int N = PIPE_N;
  const int lane = tid & 63, hi = lane >> 5, l31 = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  if (count <= 0) return;
  const int D = H * DH, half = qn.rot >> 1;
  const int qrow = wave * 32 + l31;
  // ---- loop-invariant: rotary rows of this lane's token row, LDS offsets of the fragment reads.  A thread transforms the SAME
  //      (row, channel chunk) set of K that it holds of Q -- row qrow, chunks d0 = 16 ks + 8 hi -- so one set of table rows serves both
  f32x4_t qc[4], qs[4];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    const int d0 = ks * 16 + hi * 8;
    if (d0 < qn.rot) {
      qc[ks] = *(const f32x4_t*)(qn.cs + (int64_t)qrow * half + (d0 >> 1));
      qs[ks] = *(const f32x4_t*)(qn.sn + (int64_t)qrow * half + (d0 >> 1));
    } else {
      qc[ks] = qs[ks] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    }
  }
  int ro[4];  // frag_rows(tile, base + l31, ks, hi) = tile + base * ROWB + ro[ks]   (base % 32 == 0: the swizzle term is the lane's)
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) ro[ks] = tile_off(l31, ks * 2 + hi);
  int co[2][2];  // frag_cols(tile, rbase, 32 cb, lane) halves = tile + rbase * ROWB + co[cb][0 / 1]   (rbase % 16 == 0)
  {
    const int li = lane & 15, g = lane >> 4;
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) {
        const int col = cb * 32 + (g & 1) * 16 + (li & 3) * 4, r = (g >> 1) * 4 + (li >> 2) + 8 * hh;
        co[cb][hh] = r * ROWB + (((col >> 3) ^ swz8(r)) << 4) + (col & 7) * 2;
      }
  }
  const float c = scale * LOG2E;
  // the QK-norm scales of every head in LDS behind the tile buffers (their per-item global loads would sit on the item's chain)
  float* sq_l = (float*)(smem + 4 * N * ROWB);
  float* sk_l = sq_l + D;
  for (int i = tid; i < D; i += 512) {
    sq_l[i] = qn.sq[i];
    sk_l[i] = qn.sk[i];
  }

  u32x4_t qraw[4];
  float ssq_q, ssq_k;
  u32x4_t opk[4];       // the previous item's O rows, packed: stored one item late, BEFORE the next prefetch is requested, so that the
  float lse_pend = 0.f; // wait at the top of an item (vmcnt(0): tiles + registers of this item) never waits for a store just issued
  auto store_pending = [&](int item) {
    const int b = item / H, h = item - b * H;
    bf16_t* rowp = out + ((int64_t)b * N + qrow) * (H * DH) + h * DH;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int gp = 0; gp < 2; ++gp) *(u32x4_t*)(rowp + dt * 32 + 16 * gp + 8 * hi) = opk[dt * 2 + gp];
    if (hi == 0) lse[(int64_t)item * N + qrow] = lse_pend;
  };
  auto issue_tiles = [&](int item, int buf) {
    const int b = item / H, h = item - b * H;
    const bf16_t* base = qkv + (int64_t)b * N * qn.pitch + h * DH;
    char* kt = smem + buf * (2 * N * ROWB);
    tile_dma(base + D, qn.pitch, kt, N, wave, 8, lane);
    tile_dma(base + 2 * D, qn.pitch, kt + N * ROWB, N, wave, 8, lane);
  };
  auto issue_regs = [&](int item) {
    const int b = item / H, h = item - b * H;
    const bf16_t* base = qkv + (int64_t)b * N * qn.pitch + h * DH;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) qraw[ks] = *(const u32x4_t*)(base + (int64_t)qrow * qn.pitch + ks * 16 + hi * 8);
    const float2 sq2 = *(const float2*)(qn.ssq + ((int64_t)b * N + qrow) * 2);
    ssq_q = sq2.x;
    ssq_k = sq2.y;
  };
  issue_regs(first);
  issue_tiles(first, 0);

  for (int i = 0, it = first; i < count; ++i, it += stride) {
    const int buf = i & 1;
    char* kt = smem + buf * (2 * N * ROWB);
    char* vt = kt + N * ROWB;
    const int b = it / H, h = it - b * H, bh = it;
    const int64_t tok = (int64_t)b * N + qrow;
    // the tiles and registers of THIS item were requested one item ago, before that item's main loop; nothing younger is in flight
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();  // every wave's share of the tiles has landed; every wave is done with the other buffer (and, first item, sq_l / sk_l)
    // ---- this wave's query rows: normalised + rotated in registers
    const float rq = rsqrtf(ssq_q * qn.inv_d + qn.eps);
    bf16x8_t qf[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const int d0 = ks * 16 + hi * 8;
      const u32x4_t t = qk_xform8(qraw[ks], rq, sq_l + h * DH + d0, (const float*)&qc[ks], (const float*)&qs[ks], d0 < qn.rot);
      qf[ks] = __builtin_bit_cast(bf16x8_t, t);
      if (qn.qo) *(u32x4_t*)(qn.qo + ((int64_t)bh * N + qrow) * DH + d0) = t;
    }
    if (qn.rrms && h == 0 && hi == 0) qn.rrms[tok * 2] = rq;
    // ---- K tile: in place in LDS (this thread's chunks: row qrow, the fragment slots of its q registers)
    const float rk = rsqrtf(ssq_k * qn.inv_d + qn.eps);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const int d0 = ks * 16 + hi * 8;
      char* p = kt + wave * 32 * ROWB + ro[ks];
      const u32x4_t t = qk_xform8(*(const u32x4_t*)p, rk, sk_l + h * DH + d0, (const float*)&qc[ks], (const float*)&qs[ks], d0 < qn.rot);
      *(u32x4_t*)p = t;
      if (qn.ko) *(u32x4_t*)(qn.ko + ((int64_t)bh * N + qrow) * DH + d0) = t;
    }
    if (qn.rrms && h == 0 && hi == 0) qn.rrms[tok * 2 + 1] = rk;
    if (i > 0) store_pending(it - stride);
    // ---- prefetch the next item: raw q fragments + statistics into the registers just consumed, K / V into the other buffer
    if (i + 1 < count) issue_regs(it + stride);
    __syncthreads();
    if (i + 1 < count) issue_tiles(it + stride, buf ^ 1);

    f32x16_t o[2];
#pragma unroll
    for (int r = 0; r < 16; ++r) o[0][r] = o[1][r] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;
#pragma unroll 1
    for (int kb = 0; kb < N; kb += 64) {
      // V fragments of this key block first (asm: no compiler-side wait), consumed after the softmax arithmetic
      union {
        s16x4_t h[2];
        bf16x8_t v;
      } vf[2][2][2];
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int kg2 = 0; kg2 < 2; ++kg2)
#pragma unroll
          for (int cb = 0; cb < 2; ++cb) {
            const char* pb = vt + (kb + t * 32 + kg2 * 16) * ROWB;
            vf[t][kg2][cb].h[0] = attn_lds_tr16(pb + co[cb][0]);
            vf[t][kg2][cb].h[1] = attn_lds_tr16(pb + co[cb][1]);
          }
      f32x16_t s[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
#pragma unroll
        for (int r = 0; r < 16; ++r) s[t][r] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) s[t] = MFMA(*(const bf16x8_t*)(kt + (kb + t * 32) * ROWB + ro[ks]), qf[ks], s[t]);
      }
      float mx = -INFINITY;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          s[t][r] *= c;
          mx = fmaxf(mx, s[t][r]);
        }
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float m_new = fmaxf(m_run, mx);
      const float alpha = fast_exp2(m_run - m_new);
      m_run = m_new;
      float ps = 0.f;
      float p[2][16];
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          p[t][r] = fast_exp2(s[t][r] - m_new);
          ps += p[t][r];
        }
      l_run = l_run * alpha + ps;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        o[0][r] *= alpha;
        o[1][r] *= alpha;
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int kg2 = 0; kg2 < 2; ++kg2)
#pragma unroll
          for (int cb = 0; cb < 2; ++cb) asm volatile("" : "+v"(vf[t][kg2][cb].v));  // (no MFMA on these registers above the wait)
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int kg2 = 0; kg2 < 2; ++kg2) {
          const bf16x8_t pf = pack_frag(&p[t][kg2 * 8]);
          o[0] = MFMA(vf[t][kg2][0].v, pf, o[0]);
          o[1] = MFMA(vf[t][kg2][1].v, pf, o[1]);
        }
    }
    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    const float inv = 1.0f / l_tot;
    pack_rows64(opk, o, inv);
    lse_pend = (m_run + log2f(l_tot)) * LN2;
  }
  store_pending(first + (count - 1) * stride);
}

#endif  // DIFFULAB_ATTENTION_BODY_H
