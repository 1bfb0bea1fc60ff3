"""Element-wise error bounds and poisoned buffers for the GEMM-family kernel tests (imported by the test modules; not a conftest).

A relative-L2 criterion over a large output cannot see a local error: on a 16384 x 1152 x 384 product one zeroed 8 x 16 fragment,
or a bf16 store that truncates instead of rounding, still scores < 4e-3.  Here every output element gets its own bound, derived from
what the kernel computes, and the kernel's footprint is checked bit for bit.

Reference and bound, for bf16 operands a [M, K] and b [N, K] (exact in fp64: the products of two bf16 values are exact):
    ref     = a @ b^T                                  (fp64; torch's fp64 GEMM, independent of this library)
    acc_err = c * K * 2^-24 * (|a| @ |b|^T),  c = 2
Fp32 accumulation of K terms in any order -- split-K partials, atomics and folds included -- stays within gamma_K * sum |a||b| with
gamma_K ~ K * 2^-24.  The factor 2 is margin for the MFMA unit's internal accumulation order and rounding.
Every epilogue step then adds its own term (see the functions below), and the final store adds half an ulp of |ref| + err:
2^(e - 9) for bf16 and 2^(e - 25) for f32, where 2^(e - 1) <= |ref| + err < 2^e.

The bounds of the softmax-attention kernels (forward, backward, the UNet's saved-probability forms, the fused QK-norm forward) live
in tests/attention_bounds.py, which builds on the constants, store terms and poisoned buffers of this module.
"""

from __future__ import annotations

import torch

U32 = 2.0**-24  # unit roundoff of f32
ACC_C = 2.0
BF16_POISON = 0x7FC1  # a bf16 quiet NaN with a payload no kernel produces
F32_POISON = 0x7FC1DEAD  # an f32 quiet NaN with a payload no kernel produces


# ------------------------------------------------------------------------------------------------------------------ reference + bound
def half_ulp(x: torch.Tensor, bits: int) -> torch.Tensor:
    """half an ulp of a value of magnitude x (>= 0, fp64) in a binary format with `bits` significand bits (bf16: 8, f32: 24)"""
    _, e = torch.frexp(x)  # x = m 2^e, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(x), (e - 1 - bits).to(torch.int32))


def gemm_ref(a: torch.Tensor, b: torch.Tensor, c: float = ACC_C) -> tuple[torch.Tensor, torch.Tensor]:
    """(ref, acc_err) of a [M, K] @ b [N, K]^T, fp64, on the operands' device"""
    A, B = a.double(), b.double()
    K = A.shape[1]
    return A @ B.t(), c * K * U32 * (A.abs() @ B.abs().t())


def tn_ref(a: torch.Tensor, b: torch.Tensor, init: torch.Tensor, c: float = ACC_C) -> tuple[torch.Tensor, torch.Tensor]:
    """(ref, err) of init [M, N] (f32) += a [R, M]^T @ b [R, N]: the initial value is one more addend of the f32 sum"""
    A, B, C0 = a.double(), b.double(), init.double()
    R = A.shape[0]
    return C0 + A.t() @ B, c * (R + 1) * U32 * (C0.abs() + A.abs().t() @ B.abs())


def conv_cols(x: torch.Tensor, Bn: int, H: int, W: int) -> torch.Tensor:
    """the implicit-GEMM operand of a 3x3 / pad-1 convolution over NHWC rows x [Bn*H*W, Ci]: cols[p, tap * Ci + ci], tap = 3 ky + kx"""
    Ci = x.shape[1]
    xp = torch.nn.functional.pad(x.double().reshape(Bn, H, W, Ci), (0, 0, 1, 1, 1, 1))
    taps = [xp[:, ky:ky + H, kx:kx + W, :] for ky in range(3) for kx in range(3)]
    return torch.cat(taps, dim=3).reshape(Bn * H * W, 9 * Ci)


def conv_ref(x: torch.Tensor, Bn: int, H: int, W: int, wf: torch.Tensor, c: float = ACC_C) -> tuple[torch.Tensor, torch.Tensor]:
    """(ref, acc_err) of out[p, co] = sum_{tap, ci} x[p + shift(tap), ci] wf[co, tap * Ci + ci]: K = 9 Ci"""
    return gemm_ref(conv_cols(x, Bn, H, W), wf, c)


def add_bias(ref, err, bias):
    """v = acc + bias in f32: one rounding of |acc| + |bias|"""
    bias = bias.double()
    return ref + bias, err + U32 * (ref.abs() + err + bias.abs())


def add_bias_resid(ref, err, bias=None, resid=None):
    """v = acc + bias + resid in f32, two additions in either order: two roundings of |acc| + |bias| + |resid|"""
    mag = ref.abs() + err
    if bias is not None:
        ref, mag = ref + bias.double(), mag + bias.double().abs()
    if resid is not None:
        ref, mag = ref + resid.double(), mag + resid.double().abs()
    return ref, err + 2 * U32 * mag


def silu_dev_rel(x):
    """relative error of the device silu_f(x) = x * rcp(1 + exp2(log2e * -x)) for an exact input x (fp64 magnitude |x|):
    the f32 argument of exp2 is off by <= 1.5 * 2^-24 |x log2 e| (rounded log2 e, rounded product) -> 1.5 |x| 2^-24 relative in exp2,
    v_exp_f32 and v_rcp_f32 1 ulp (2 * 2^-24) each, the add and the multiply 2^-24 each"""
    return (1.5 * x.abs() + 6.0) * U32


def silu(ref, err):
    """z = silu(v): |silu'| <= 1.1 times the input error, plus the device's own error on the computed input"""
    s = ref * torch.sigmoid(ref)
    e = 1.1 * err + silu_dev_rel(ref.abs() + err) * (s.abs() + 1.1 * err) + 2.0**-126
    return s, e


def swiglu(r1, e1, r3, e3):
    """h = silu(x1) * x3 in f32 from the accumulators"""
    s, es = silu(r1, e1)
    h = s * r3
    return h, es * r3.abs() + s.abs() * e3 + es * e3 + U32 * (h.abs() + es * r3.abs() + s.abs() * e3)


def gate_resid(ref, err, resid, gate=None):
    """v = resid + gate * z (gate None: resid + z) in f32: |gate| err_z plus one f32 rounding of each term"""
    r = resid.double()
    if gate is not None:
        g = gate.double()
        gz, e = g * ref, g.abs() * err
        e = e + U32 * (gz.abs() + e)
    else:
        gz, e = ref, err
    out = r + gz
    return out, e + U32 * (out.abs() + e)


def store_bf16(ref, err):
    return err + half_ulp(ref.abs() + err, 8)


def store_f32(ref, err):
    return err + half_ulp(ref.abs() + err, 24)


def assert_within(out: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor, tile=(128, 128), what: str = "") -> None:
    """every element of `out` within `bound` of `ref` (NaN fails); the message names the number of violations, the worst element,
    its output tile (tile = the kernel's BM x BN) and its 16 x 16 fragment"""
    assert out.shape == ref.shape == bound.shape, (out.shape, ref.shape, bound.shape)
    o = out.to(ref.device).double()
    d = (o - ref).abs()
    bad = ~(d <= bound)
    n = int(bad.sum())
    if n == 0:
        return
    excess = torch.where(bad, torch.nan_to_num(d - bound, nan=float("inf")), torch.full_like(d, -float("inf")))
    idx = int(excess.reshape(-1).argmax())
    cols = out.shape[1] if out.dim() == 2 else 1
    r, c = divmod(idx, cols)
    ov, rv, bv = float(o.reshape(-1)[idx]), float(ref.reshape(-1)[idx]), float(bound.reshape(-1)[idx])
    raise AssertionError(
        f"{what}: {n} of {out.numel()} elements outside their bound; worst [{r}, {c}] = {ov!r}, ref {rv!r}, |diff| {abs(ov - rv):.3e} > "
        f"bound {bv:.3e}; output tile ({r // tile[0]}, {c // tile[1]}) of {tile[0]}x{tile[1]}, 16x16 fragment ({r // 16}, {c // 16})")


def rel_l2(out, ref) -> float:
    """the suite's older criterion: relative L2 error over the whole output"""
    o, r = out.double().to(ref.device), ref
    return float((o - r).norm() / r.norm().clamp_min(1e-30))


# ------------------------------------------------------------------------------------------------------------------ poisoned buffers
def _int_view(t: torch.Tensor) -> torch.Tensor:
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


def poison_value(dtype) -> int:
    return BF16_POISON if dtype == torch.bfloat16 else F32_POISON


def poison_(t: torch.Tensor) -> torch.Tensor:
    _int_view(t).fill_(poison_value(t.dtype))
    return t


def is_poison(t: torch.Tensor) -> torch.Tensor:
    return _int_view(t) == poison_value(t.dtype)


class Guarded:
    """a [rows, cols] window inside a poisoned [top + rows + bottom, ld] allocation: `left` guard columns before the window, the rest
    of the row after it (ld = left + cols + right rounded up to a multiple of 8, or `ld` as given), guard rows above and below.
    init None: the window starts poisoned too (= semantics: afterwards it must be finite); else it starts from `init` (+= semantics)."""

    def __init__(self, rows, cols, dtype, device, left=8, right=8, top=1, bottom=2, ld=None, init=None):
        ld = ld if ld is not None else (left + cols + right + 7) // 8 * 8
        assert ld >= left + cols
        self.buf = poison_(torch.empty(top + rows + bottom, ld, dtype=dtype, device=device))
        self.win = self.buf[top:top + rows, left:left + cols]
        self.mask = torch.ones(self.buf.shape, dtype=torch.bool, device=device)
        self.mask[top:top + rows, left:left + cols] = False
        if init is not None:
            self.win.copy_(init)

    def check(self, what: str = "") -> None:
        check_footprint(self.buf, self.mask, self.win, what)


def check_footprint(buf, guard_mask, win, what: str = "") -> None:
    """every guard element bit-identical to the poison, every window element finite"""
    hit = guard_mask & ~is_poison(buf)
    n = int(hit.sum())
    if n:
        r, c = divmod(int(hit.reshape(-1).nonzero()[0]), buf.shape[1])
        raise AssertionError(f"{what}: {n} guard elements written, first at buffer [{r}, {c}]")
    fin = torch.isfinite(win.float())
    n = int((~fin).sum())
    if n:
        r, c = divmod(int((~fin).reshape(-1).nonzero()[0]), win.shape[1])
        raise AssertionError(f"{what}: {n} window elements not finite (unwritten, or NaN from a read past the operand), first at [{r}, {c}]")


def operand(values: torch.Tensor, ld: int, col0: int = 0, guard_rows: int = 2) -> torch.Tensor:
    """values [rows, cols] placed at column col0 of a poisoned [rows + guard_rows, ld] bf16 buffer: the returned view has row stride
    ld, and a kernel that reads past its row (or below the last row) reads NaN"""
    rows, cols = values.shape
    assert col0 + cols <= ld
    buf = poison_(torch.empty(rows + guard_rows, ld, dtype=values.dtype, device=values.device))
    v = buf[:rows, col0:col0 + cols]
    v.copy_(values)
    return v
