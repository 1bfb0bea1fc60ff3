"""fp64 references, element-wise bounds and input families for the optimizer-step, weight-cast and noising kernels of
csrc/elementwise.hip (imported by the test modules; not a conftest).  Builds on tests/elementwise_bounds.py and tests/f32_bounds.py.

One function per operation returns {output: (ref, bound)} in fp64, bound None where the kernel only moves or rounds data and must
agree bit for bit (the casts and layouts: their references are bit patterns in integer tensors).

Scalars enter as the C ABI receives them: every `float` argument rounded to f32 first; lr / bias_corr1 and 1 / sqrt(bias_corr2) formed
in double from the f32 arguments and rounded, as the launchers do; 1 - beta as the f32 subtraction.  So the references carry no
error of their own against the kernels' scalars, and the bounds hold only the kernels' own roundings.

Bounds count the roundings of the kernel source for either contraction choice (a * b + c as one fma or as a rounded product and a
rounded sum), u = 2^-24, first order in u; the factor SO = 1 + 2^-20 covers the higher orders and 2^-149 the subnormal spacing.
Nothing here was fitted to a GPU result.  The counts, term by term, stand next to the code.

The input families and case tables of tests/test_step_paths_gpu.py live here too, generated on the CPU from fixed seeds, so that
tests/test_step_bounds_host.py can show on the very same inputs which wrong kernels the bounds reject.
"""

from __future__ import annotations

import math

import numpy as np
import torch

import elementwise_bounds as eb
import f32_bounds as fb

U = eb.U32
TINY = fb.TINY
SO = 1.0 + 2.0**-20  # second and higher orders of every first-order count below
F32 = torch.float32
EW_CAP = 2048 * 256  # ew_grid: at most 2048 workgroups of 256 threads, grid-stride beyond


def f32c(x: float) -> float:
    """the f32 value of a scalar, as a python float (what a `float` argument of the ABI holds)"""
    return float(np.float32(x))


def _bound(first_order):
    """a first-order count -> the bound of an f32 result: higher orders, the subnormal spacing"""
    return SO * first_order + TINY


# ------------------------------------------------------------------------------------------------------------------ AdamW
# hyperparameter sets of the GPU table: (name, lr, betas, eps, weight_decay, step, grad_scale, coef); coef is read by the _clip forms
ADAMW_HYPERS = (
    ("default-step1", 1e-3, (0.9, 0.999), 1e-8, 0.01, 1, 1.0, 1.0),
    ("default-step1000", 1e-3, (0.9, 0.999), 1e-8, 0.01, 1000, 1.0, 1.0),
    ("visible", 0.1, (0.875, 1.0 - 2.0**-10), 1e-3, 0.3, 3, 1.0, 1.0),  # weight-decay order and the place of eps show
    ("wd0", 1e-3, (0.9, 0.999), 1e-8, 0.0, 10, 1.0, 1.0),
    ("visible-gs0.5", 0.1, (0.875, 1.0 - 2.0**-10), 1e-3, 0.3, 3, 0.5, 1.0),
    ("default-gs0.5-coef0.37", 1e-3, (0.9, 0.999), 1e-8, 0.01, 1, 0.5, 0.37),
    ("visible-coef0.37", 0.1, (0.875, 1.0 - 2.0**-10), 1e-3, 0.3, 3, 1.0, 0.37),
)
ADAMW_SMALL_N = (1, 2, 3, 4, 5, 7, 1023, 1027)  # tail only, body only, both
ADAMW_PLAIN_BIG_N = 4 * EW_CAP + 23  # the second grid-stride trip of the float4 loop and a 3-element tail
ADAMW_DEV_BIG_N = EW_CAP + 77


def adamw_scalars(lr, betas, eps, wd, step, grad_scale=1.0, coef=None) -> dict:
    """the f32 scalars of one step as ops.adamw_step* passes them and as the launchers derive them; coef None: a form without clipping"""
    S = dict(lr=f32c(lr), b1=f32c(betas[0]), b2=f32c(betas[1]), eps=f32c(eps), wd=f32c(wd), bc1=f32c(1.0 - betas[0]**step),
             bc2=f32c(1.0 - betas[1]**step), grad_scale=f32c(grad_scale), coef=None if coef is None else f32c(coef), step=step)
    S["ilr"] = f32c(S["lr"] / S["bc1"])  # (float)((double)lr / (double)bias_corr1)
    S["isb"] = f32c(1.0 / math.sqrt(S["bc2"]))  # (float)(1.0 / sqrt((double)bias_corr2))
    S["omb1"], S["omb2"] = f32c(1.0 - S["b1"]), f32c(1.0 - S["b2"])  # 1.0f - beta: the exact difference, rounded once
    S["gs"] = S["grad_scale"] if coef is None else f32c(S["grad_scale"] * S["coef"])  # grad_scale * *coef: an exact product, rounded once
    return S


def adamw_hyper(S: dict) -> torch.Tensor:
    """the f32 [8] device scalars of dl_adamw_step_dev*: hyper[7] is grad_scale, the kernel multiplies the coefficient in"""
    return torch.tensor([S["lr"], S["b1"], S["b2"], S["eps"], S["wd"], S["ilr"], S["isb"], S["grad_scale"]], dtype=F32)


def adamw_inputs(n: int, seed: int = 0):
    """(p, g, m, v) f32 [n] on the CPU: every third gradient of magnitude 1e-7 beside O(1) ones (eps dominates those denominators),
    every second first moment of the sign opposite to its gradient (cancellation in m'), every fifth second moment zero"""
    gen = torch.Generator().manual_seed(1000 + seed)
    i = torch.arange(n)
    g = torch.randn(n, generator=gen)
    g = torch.where(g == 0, torch.full_like(g, 0.5), g)
    g = torch.where(i % 3 == 1, g * 1e-7, g)
    mag = torch.rand(n, generator=gen) * 0.9 + 0.1
    m = torch.where(i % 2 == 0, -torch.sign(g) * mag, 0.1 * torch.randn(n, generator=gen))
    v = torch.where(i % 5 == 0, torch.zeros(n), torch.rand(n, generator=gen) * 1e-2)
    p = torch.randn(n, generator=gen)
    return p, g, m, v


def adamw_ref(p, g, m, v, S: dict) -> dict:
    """torch.optim.AdamW's rule with the f32 scalars S, in fp64:
        gr = g gs;  m' = b1 m + (1 - b1) gr;  v' = b2 v + (1 - b2) gr^2;  p' = (1 - lr wd) p - ilr m' / (sqrt(v') isb + eps)"""
    P, G, M, V = (t.double() for t in (p, g, m, v))
    gr = G * S["gs"]  # kernel: 1 rounding (relative u)
    a, b = S["b1"] * M, S["omb1"] * gr
    m1 = a + b
    # b1 m: 1 (product); (1 - b1) gr: 1 (gr) + 1 (product); the sum: 1, of |m'| <= |a| + |b|  ->  2 |a| + 3 |b| <= 3 (|a| + |b|)
    E_m = 3 * U * (a.abs() + b.abs())
    v1 = S["omb2"] * gr * gr + S["b2"] * V
    # (1 - b2) gr gr: 2 (gr, twice) + 2 (two products); b2 v: 1; the sum: 1; every term >= 0, so relative to v': 5
    E_v = 5 * U * v1
    den = v1.sqrt() * S["isb"] + S["eps"]
    # sqrtf: 5 / 2 (v') + 1/2 (correctly rounded, fb.SQRT_ULP) = 3; times isb: 1; the sum with eps >= 0: 1; margin 1  ->  6 denom
    E_d = 6 * U * den
    q = m1 / den
    # m' / denom: E_m / denom + 6 |q| (denom) + 1 |q| (the division, correctly rounded: fb.DIV_ULP)
    E_q = E_m / den + 7 * U * q.abs()
    decay = 1.0 - S["lr"] * S["wd"]
    p1 = decay * P - S["ilr"] * q
    # decay p: 2 (lr wd, 1 - lr wd; one as an fma) + 1 (product), decay <= 1; ilr q: ilr E_q + 1 (product); the difference: 1
    E_p = 3 * U * P.abs() * max(1.0, abs(decay)) + S["ilr"] * E_q + U * (S["ilr"] * q).abs() + U * p1.abs()
    out = {}
    for k, r, e in (("p", p1, E_p), ("m", m1, E_m), ("v", v1, E_v)):
        e = _bound(e)
        out[k] = (r, e + eb.half_ulp(r.abs() + e, 24))  # the f32 store
    return out


# ------------------------------------------------------------------------------------------------------------------ noising, EMA
FLOW_VEC_SHAPES = ((1, 4), (5, 4), (3, 1024), (3, 700_004))  # (batch, chw); the last: 525 003 float4s > EW_CAP
FLOW_SCALAR_SHAPES = ((1, 1), (5, 1), (3, 35), (3, 174_765))  # the last: 524 295 elements > EW_CAP
EMA_N = (1, 257, EW_CAP + 77)
EMA_BETAS = (0.9, 0.9999, 0.1)


def sample_times(batch: int) -> torch.Tensor:
    """per-sample t in (0, 1), f32, neighbours at least 0.1 apart: a neighbour's t moves z by ~ 0.1 |eps - x|"""
    return ((torch.arange(batch, dtype=torch.float64) * 0.37 + 0.11) % 1.0).to(F32)


def sample_steps(batch: int, T: int) -> torch.Tensor:
    """per-sample integer steps, int32: 0 and T - 1 first, neighbours never equal"""
    t = (torch.arange(batch, dtype=torch.int64) * 389 + 3) % T
    t[0] = 0
    if batch > 1:
        t[1] = T - 1
    return t.to(torch.int32)


def noise_inputs(batch: int, chw: int, seed: int = 0):
    gen = torch.Generator().manual_seed(2000 + seed)
    return torch.randn(batch, chw, generator=gen), torch.randn(batch, chw, generator=gen)


def flow_ref(x, e, t) -> dict:
    """z = (1 - t) x + t eps over x, eps [batch, chw], t [batch]"""
    X, E, tt = x.double(), e.double(), t.double()[:, None]
    a, b = (1.0 - tt) * X, tt * E
    z = a + b
    # (1 - t) x: 1 (the f32 difference 1 - t) + 1 (product); t eps: 1; the sum: 1 (fused with one product or not)
    return {"z": (z, _bound(U * (2 * a.abs() + b.abs() + z.abs())))}


def ddpm_ref(x, e, t, sqrt_ab, ab) -> dict:
    """x_t = sqrt_ab[t] x + sqrtf(1 - ab[t]) eps, the tables f32, the square root taken in f32"""
    X, E = x.double(), e.double()
    ti = t.long()
    ca, omab = sqrt_ab.double()[ti][:, None], (1.0 - ab.double()[ti])[:, None]
    a, b = ca * X, omab.sqrt() * E
    o = a + b
    # ca x: 1; sqrtf(1 - ab) eps: 1/2 (the f32 difference, under the root) + 2 (fb.SQRT_ULP = 1 ulp = 2 u) + 1 (product); the sum: 1
    return {"xt": (o, _bound(U * (a.abs() + (0.5 + 2 * fb.SQRT_ULP + 1) * b.abs() + o.abs())))}


def ema_weight(beta: float) -> float:
    """dl_ema_update's w: 1.0f - beta evaluated in f32"""
    return f32c(1.0 - f32c(beta))


def ema_ref(ema, p, beta: float) -> dict:
    """ema' = ema + w (p - ema)"""
    E, P, w = ema.double(), p.double(), ema_weight(beta)
    d = w * (P - E)
    o = E + d
    # w (p - e): 1 (the difference) + 1 (product); the sum: 1 (fused with the product or not)
    return {"ema": (o, _bound(U * (2 * d.abs() + o.abs())))}


# ------------------------------------------------------------------------------------------------------------------ casts
F32_LOW_HALVES = (0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF)  # exact, just above, just below a tie, a tie, just above a tie, all ones


def f32_patterns() -> torch.Tensor:
    """every 16-bit high half x F32_LOW_HALVES as f32 [65536 * 6]: ties on even and odd mantissas, carries into the exponent and into
    infinity, the largest finite values, +-0, subnormals, +-inf and NaNs of every payload class"""
    hi = torch.arange(65536, dtype=torch.int64)[:, None] << 16
    lo = torch.tensor(F32_LOW_HALVES, dtype=torch.int64)[None, :]
    return from_bits32((hi | lo).reshape(-1))


def bf16_patterns() -> torch.Tensor:
    """all 65 536 bf16 values, in order of their bit pattern"""
    return from_bits16(torch.arange(65536, dtype=torch.int64))


def from_bits32(b: torch.Tensor) -> torch.Tensor:
    b = b.to(torch.int64) & 0xFFFFFFFF
    return torch.where(b >= 2**31, b - 2**32, b).to(torch.int32).view(F32)


def from_bits16(b: torch.Tensor) -> torch.Tensor:
    b = b.to(torch.int64) & 0xFFFF
    return torch.where(b >= 2**15, b - 2**16, b).to(torch.int16).view(torch.bfloat16)


def bits32(t: torch.Tensor) -> torch.Tensor:
    """the bit patterns of an f32 tensor as non-negative int64"""
    return t.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF


def bits16(t: torch.Tensor) -> torch.Tensor:
    """the bit patterns of a bf16 tensor as non-negative int64"""
    return t.contiguous().view(torch.int16).to(torch.int64) & 0xFFFF


def f32_to_bf16_bits(x: torch.Tensor):
    """round-to-nearest-even on the bit pattern, in integer arithmetic (no library cast): -> (bf16 patterns int64, NaN mask).
    Adding 0x7FFF + (the lowest kept bit) carries into the kept half exactly when the dropped half is above a tie, or on a tie
    with an odd kept half; the carry runs on into the exponent and, from the largest finite values, into infinity, as IEEE
    rounding does.  f32 subnormals round the same way (bf16 has the exponent range of f32).  A NaN must stay a NaN, its
    sign and payload are not compared."""
    b = bits32(x)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) & 0xFFFF
    return r, (b & 0x7FFFFFFF) > 0x7F800000


def bf16_to_f32_bits(x: torch.Tensor) -> torch.Tensor:
    """a shift: exact for every pattern, NaN payloads included"""
    return bits16(x) << 16


def cast_mismatch(got: torch.Tensor, src: torch.Tensor) -> int:
    """elements of the bf16 tensor `got` that are not the rounding of the f32 tensor `src` (same shape): bit-exact, any NaN for a NaN"""
    want, nan = f32_to_bf16_bits(src)
    g = bits16(got).to(want.device)
    ok = torch.where(nan, (g & 0x7FFF) > 0x7F80, g == want)
    return int((~ok).sum())


def weight_input(R: int, C: int, seed: int = 0) -> torch.Tensor:
    """f32 [R, C], N(0, 1) with the dropped half of every third element set to a tie (0x8000) and of every third to above a tie
    (0xC000): a store that truncates, or that rounds ties away from zero, differs from round-to-nearest-even on this data (on a
    tie under an even kept half only the second does, above a tie only the first: no single element shows both)"""
    gen = torch.Generator().manual_seed(3000 + seed)
    b = bits32(torch.randn(R * C, generator=gen))
    i = torch.arange(R * C)
    b = torch.where(i % 3 == 0, (b & 0xFFFF0000) | 0x8000, b)
    b = torch.where(i % 3 == 1, (b & 0xFFFF0000) | 0xC000, b)
    return from_bits32(b).reshape(R, C)


def ddpm_tables(T: int):
    """(sqrt_alphas_bar, alphas_bar) f32 [T] of the linear schedule: 1000 training steps, respaced to T where T < 1000"""
    from oracle import diffusion as od

    G = od.GaussianTables(1000, T)
    return G.sqrt_alphas_bar.float(), G.alphas_bar.float()


# ------------------------------------------------------------------------------------------------------------------ layouts
CAST_WEIGHT_SHAPES = ((1, 1), (31, 33), (100, 72), (64, 64), (37, 5))
CAST_WEIGHT_PADS = ((0, 0), (8, 8), (40, 40), (0, 40), (40, 0))  # (ld_dst - C, ld_t - R): inside the last tile, whole extra tiles
SWIGLU_SHAPES = ((16, 8, 8), (48, 72, 104), (272, 960, 968))  # (F, C, ld); the last: 2 F ld = 526 592 > EW_CAP
# the 7-entry CastTable (an odd count for the binary search), all five destination combinations:
# (R, C, ld_dst | None, ld_t | None, ld_swiglu | None); which leading dimension sets the tile grid is noted
CAST_TABLE = (
    (1, 1, 8, None, None),  # dst
    (37, 5, None, 77, None),  # dst_t; ld_t = R + 40 sets the tile rows
    (100, 72, 80, 100, None),  # dst + dst_t
    (96, 40, 40, None, 80),  # dst + dst_swiglu; ld_dst = C, ld_swiglu = C + 40 sets the tile columns
    (64, 136, 176, 72, 136),  # all three; ld_dst = C + 40 sets the tile columns
    (31, 33, 33, 71, None),  # dst + dst_t; ld_t = R + 40
    (64, 64, 64, None, 64),  # dst + dst_swiglu
)


def plain_bits(src: torch.Tensor, ld: int) -> torch.Tensor:
    """the plain bf16 copy [R, ld] of src [R, C] as bit patterns: +0 in every padding column c in [C, ld)"""
    R, C = src.shape
    out = torch.zeros(R, ld, dtype=torch.int64, device=src.device)
    out[:, :C] = f32_to_bf16_bits(src)[0]
    return out


def transposed_bits(src: torch.Tensor, ld_t: int) -> torch.Tensor:
    """the transposed bf16 copy [C, ld_t]: +0 in the padding columns r in [R, ld_t)"""
    R, C = src.shape
    out = torch.zeros(C, ld_t, dtype=torch.int64, device=src.device)
    out[:, :R] = f32_to_bf16_bits(src)[0].t()
    return out


def swiglu_rows(F: int) -> torch.Tensor:
    """source row of every destination row of the SwiGLU layout over src [2 F, C] = [x1 rows | x3 rows]: 32-row groups, the 16 x1 rows
    of hidden units 16 q .. 16 q + 15, then the 16 x3 rows of the same units"""
    assert F % 16 == 0
    n = torch.arange(2 * F)
    q, s = n // 32, n % 32
    return torch.where(s < 16, 16 * q + s, F + 16 * q + (s - 16))


def swiglu_bits(src: torch.Tensor, ld: int) -> torch.Tensor:
    """the row-permuted bf16 copy [2 F, ld] of src [2 F, C]"""
    return plain_bits(src, ld)[swiglu_rows(src.shape[0] // 2).to(src.device)]
