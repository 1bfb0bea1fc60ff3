"""fp64 references and element-wise error bounds for every dl_f32_* entry point of csrc/f32.hip (imported by the test modules; not
a conftest).  Builds on tests/elementwise_bounds.py: the same constants, store terms and poisoned buffers.

Operands are f32, so every product of two operands is exact in fp64 and torch's fp64 arithmetic is the reference.  A bound is
assembled from the steps the kernel performs, one named term per rounding, with the class V below: a V carries the fp64 value of an
intermediate and a bound on the distance of the kernel's f32 intermediate from it.  The rules:

  rnd        one f32 rounding of a computed value: half an ulp of |ref| + err (eb.store_f32), plus the subnormal spacing 2^-149.
             a * b + c may be contracted into one fma by the compiler: two roundings bound one.
  add / sub / mul      the operands' errors carried through (first and second order), then rnd
  fsum       a sum of n terms through a chain of at most `depth` f32 additions: sum of the terms' errors + ACC_C depth 2^-24 sum |term|.
             Where a kernel fixes the order the depth is stated (row kernels: 2 inside a float4 + FR_NJ chunks + 6 tree levels = 12);
             where it does not, depth = n (gamma_n, order-free), as for the GEMM: ACC_C K 2^-24 |a| . |b|, splits and fold included.
  library functions    the argument's error through the derivative (taken at its worst over the argument's interval), plus the
             measured allowance below in ulps of the result.  Results below the normal range get 2^-126 (flush) on top; where
             expf overflows (silu at x < -88.7) the f32 divisor is inf and the quotient 0: the whole (< 2.7e-37) value is allowed.
  given operands       a backward takes the saved f32 statistics (mean, rstd, rrms, probabilities) as operands: that is the kernels'
             contract, they never recompute them.

No term absorbs what a formula would owe to itself: the variance bounds hold the CENTRED second moment only (the mean's error enters
squared: the cross term vanishes), so a one-pass variance fails on the offset rows; softmax bounds hold nothing for a missing max
subtraction.  Pure data movement (restore, pick / stuff / expand, layout, copy2d, patchify, im2col and the zeros they write) has no
bound: it is compared bit for bit (bound None).

Library-function allowances.  Measured on the MI355X by scripts/f32_libm_ulp.hip (built with the flags of csrc/Makefile; every third
f32 bit pattern of the argument range, 1.1e8 .. 4.5e8 arguments per function, against fp64); the constant is twice the observed
maximum, rounded up to a whole ulp; none may exceed 8:

    function     range swept            measured max     constant
    expf         [-104, 88]             1.0000 ulp       EXP_ULP  = 2     (the maximum sits at x = -103.28, below the normal range)
    erff         [-24, 24]              1.5091 ulp       ERF_ULP  = 4
    sinf         [0, 1000]              1.5760 ulp       SIN_ULP  = 4
    cosf         [0, 1000]              1.5766 ulp       COS_ULP  = 4
    sqrtf        [2^-40, 2^40]          0.5000 ulp       SQRT_ULP = 1     (correctly rounded)
    1.0f / x     [2^-40, 2^40]          0.5000 ulp       DIV_ULP  = 1     (correctly rounded)
    x / y        [2^-40, 2^40], +-      0.5000 ulp       DIV_ULP  = 1
"""

from __future__ import annotations

import math

import torch

import elementwise_bounds as eb

U = eb.U32
ACC_C = eb.ACC_C
EXP_ULP, ERF_ULP, SIN_ULP, COS_ULP, SQRT_ULP, DIV_ULP = 2, 4, 4, 4, 1, 1
ULP_CAP = 8
TINY = 2.0**-149  # spacing of the f32 subnormals
FLUSH = 2.0**-126  # a library result below the normal range may be flushed
F32_MAX = 3.4028234663852886e38
ROW_DEPTH = 2 + 4 + 6  # fr_sum: (v0 + v1) + (v2 + v3), FR_NJ = 4 chunks per lane in order, 6 levels of the wave tree
LN_EPS = 1e-6
QK_EPS = 1e-6
GN_EPS = 1e-5
F32 = torch.float32


def f32c(x: float) -> float:
    """the f32 value of a constant, as a python float"""
    return float(torch.tensor(x, dtype=F32))


# ------------------------------------------------------------------------------------------------------------------ value + error
class V:
    """ref: fp64 value; err: bound (fp64, >= 0) on |kernel's f32 intermediate - ref|"""

    def __init__(self, ref, err=None):
        self.ref = ref
        self.err = torch.zeros_like(ref) if err is None else err

    def map(self, fn):
        """pure data movement (indexing, reshape, expand) of value and error alike"""
        return V(fn(self.ref), fn(self.err))

    @property
    def mag(self):
        return self.ref.abs() + self.err

    def pair(self):
        return self.ref, self.err


def exact(t) -> V:
    return V(t.double())


def const(x: float, like: V) -> V:
    return V(torch.full_like(like.ref, x))


def half_ulp(x):
    """eb.half_ulp for f32, with half_ulp(0) = 0: an exact zero stays exact"""
    return torch.where(x == 0, torch.zeros_like(x), eb.half_ulp(x, 24))


def rnd(v: V) -> V:
    """eb.store_f32 with an exact zero kept exact, plus the subnormal spacing where anything was computed"""
    m = v.mag
    return V(v.ref, v.err + half_ulp(m) + TINY * (m > 0))


def ulps(v: V, n: int) -> V:
    """the result of a library function: n ulps of the result on top of err, and the flush allowance"""
    return V(v.ref, v.err + 2 * n * half_ulp(v.mag) + FLUSH)


def add(a: V, b: V) -> V:
    return rnd(V(a.ref + b.ref, a.err + b.err))


def sub(a: V, b: V) -> V:
    return rnd(V(a.ref - b.ref, a.err + b.err))


def mul(a: V, b: V) -> V:
    return rnd(V(a.ref * b.ref, a.ref.abs() * b.err + b.ref.abs() * a.err + a.err * b.err))


def neg(a: V) -> V:
    return V(-a.ref, a.err)


def scale2(a: V, p: float) -> V:
    """times a power of two: exact"""
    return V(a.ref * p, a.err * abs(p))


def fsum(v: V, dim, depth: int, keepdim=False) -> V:
    """sum over `dim` through at most `depth` f32 additions per term"""
    r = v.ref.sum(dim, keepdim=keepdim)
    e = v.err.sum(dim, keepdim=keepdim) + ACC_C * depth * U * v.mag.sum(dim, keepdim=keepdim) + TINY
    return V(r, e)


def matmul(a: V, b: V) -> V:
    """a [.., M, K] @ b [.., K, N] on the f32 matrix unit: the operands' errors + ACC_C K 2^-24 |a| . |b| in any order"""
    K = a.ref.shape[-1]
    e = a.ref.abs() @ b.err + a.err @ b.ref.abs() + a.err @ b.err + ACC_C * K * U * (a.mag @ b.mag) + TINY
    return V(a.ref @ b.ref, e)


def rcp(a: V) -> V:
    """1.0f / a"""
    lo = (a.ref.abs() - a.err).clamp_min(0.0)
    e = torch.where(lo > 0, a.err / (a.ref.abs() * lo), torch.full_like(lo, float("inf")))
    e = torch.where(a.err == 0, torch.zeros_like(e), e)
    e = e + torch.where(a.mag >= F32_MAX, (1.0 / a.ref).abs(), torch.zeros_like(e))  # the f32 divisor is inf: the quotient is 0
    return ulps(V(1.0 / a.ref, e), DIV_ULP)


def div(a: V, b: V) -> V:
    """a / b as one division"""
    lo = (b.ref.abs() - b.err).clamp_min(0.0)
    q = a.ref / b.ref
    e = torch.where(lo > 0, (a.err + q.abs() * b.err) / lo, torch.full_like(lo, float("inf")))
    e = torch.where((a.err == 0) & (b.err == 0), torch.zeros_like(e), e)
    e = e + torch.where(b.mag >= F32_MAX, q.abs(), torch.zeros_like(e))  # the f32 divisor is inf (expf overflow): the quotient is 0
    return ulps(V(q, e), DIV_ULP)


def sqrt_(a: V) -> V:
    lo = (a.ref - a.err).clamp_min(TINY)
    return ulps(V(a.ref.sqrt(), a.err / (2.0 * lo.sqrt())), SQRT_ULP)


def exp_(a: V) -> V:
    r = a.ref.exp()
    return ulps(V(r, r * torch.expm1(a.err)), EXP_ULP)


def erf_(a: V) -> V:
    z = (a.ref.abs() - a.err).clamp_min(0.0)
    return ulps(V(torch.erf(a.ref), 2.0 / math.sqrt(math.pi) * torch.exp(-z * z) * a.err), ERF_ULP)


def sin_(a: V) -> V:
    return ulps(V(a.ref.sin(), (a.ref.cos().abs() + a.err).clamp_max(1.0) * a.err), SIN_ULP)


def cos_(a: V) -> V:
    return ulps(V(a.ref.cos(), (a.ref.sin().abs() + a.err).clamp_max(1.0) * a.err), COS_ULP)


def sigmoid_(x: V) -> V:
    """1.0f / (1.0f + expf(-x))"""
    return rcp(add(const(1.0, x), exp_(neg(x))))


def silu_(x: V) -> V:
    """silu32: x / (1.0f + expf(-x))"""
    return div(x, add(const(1.0, x), exp_(neg(x))))


def dsilu_(x: V) -> V:
    """dsilu32: s (1 + x (1 - s)), s = 1 / (1 + expf(-x))"""
    s = sigmoid_(x)
    one = const(1.0, x)
    return mul(s, add(one, mul(x, sub(one, s))))


def out(v: V):
    return v.ref, v.err


def bits(t):
    """a bit-for-bit expectation: (f32 tensor, None)"""
    return t, None


def _invn(n: int, like: V) -> V:
    """1.0f / (float)n"""
    return rcp(const(float(n), like)) if n & (n - 1) else const(1.0 / n, like)


# ------------------------------------------------------------------------------------------------------------------ GEMM
def gemm_ref(a, b, alpha=1.0, bias=None, silu=False, c0=None, want_pre=False):
    """a [M, K], b [N, K] f32 (the logical operands, whatever their layout): C = act(alpha a b^T + bias) (+ c0); pre = before act"""
    acc = matmul(exact(a), exact(b).map(lambda t: t.t()))
    v = acc if alpha == 1.0 else mul(acc, const(f32c(alpha), acc))
    if bias is not None:
        v = add(v, exact(bias).map(lambda t: t[None, :].expand_as(v.ref)))
    res = {}
    if want_pre:
        res["pre_out"] = out(v)
    if silu:
        v = silu_(v)
    if c0 is not None:
        v = add(v, exact(c0))
    res["C"] = out(v)
    return res


# ------------------------------------------------------------------------------------------------------------------ LayerNorm + modulate
def _rows_mod(t, rows_per_mod, M):
    """[G, D] modulation rows -> [M, D]"""
    return t.repeat_interleave(rows_per_mod, 0)[:M]


def ln_fwd_ref(x, w, b, scale, shift, rows_per_mod, eps, t=None, gate=None):
    """x [M, D]; scale / shift / gate [G, D]; -> out, mean, rstd (+ x_out)"""
    M, D = x.shape
    xv = exact(x)
    res = {}
    if t is not None:
        xv = add(xv, mul(exact(t), exact(_rows_mod(gate, rows_per_mod, M))))
        res["x_out"] = out(xv)
    invD = _invn(D, V(xv.ref[:, :1]))
    mu = mul(fsum(xv, 1, ROW_DEPTH, keepdim=True), invD)
    d = sub(xv, mu.map(lambda u: u.expand(M, D)))
    # the variance sees the centred values with their OWN rounding; the mean's error enters squared (the cross term vanishes)
    dref = xv.ref - mu.ref
    d_own = rnd(V(dref, xv.err))
    var = mul(fsum(mul(d_own, d_own), 1, ROW_DEPTH, keepdim=True), invD)
    var = V(var.ref, var.err + mu.err.square() + 2 * mu.err * xv.err.mean(1, keepdim=True))
    rs = rcp(sqrt_(add(var, const(f32c(eps), var))))
    y = mul(d, rs.map(lambda u: u.expand(M, D)))
    if w is not None:
        y = add(mul(y, exact(w).map(lambda u: u[None].expand(M, D))), exact(b).map(lambda u: u[None].expand(M, D)))
    sc, sh = exact(_rows_mod(scale, rows_per_mod, M)), exact(_rows_mod(shift, rows_per_mod, M))
    o = add(mul(y, add(const(1.0, sc), sc)), sh)
    res.update(out=out(o), mean=out(V(mu.ref[:, 0], mu.err[:, 0])), rstd=out(V(rs.ref[:, 0], rs.err[:, 0])))
    return res


def ln_bwd_ref(dout, x, w, b, scale, rows_per_mod, mean, rstd, dres=None, want_dwb=False, gate_t=None, gate=None):
    """the backward from the f32 statistics as given; -> dx, dscale, dshift [G, D] (+ dwb [G, 2, D], dt, dgate)"""
    M, D = x.shape
    G = M // rows_per_mod
    ex = lambda u: exact(u).map(lambda v: v[None].expand(M, D))  # noqa: E731
    col = lambda u: exact(u).map(lambda v: v[:, None].expand(M, D))  # noqa: E731
    d, xv = exact(dout), exact(x)
    sc = exact(_rows_mod(scale, rows_per_mod, M))
    one = const(1.0, d)
    xh = mul(sub(xv, col(mean)), col(rstd))
    dy = mul(d, add(one, sc))
    if w is not None:
        dy = mul(dy, ex(w))
    invD = _invn(D, V(d.ref[:, :1]))
    m1 = mul(fsum(dy, 1, ROW_DEPTH, keepdim=True), invD).map(lambda u: u.expand(M, D))
    m2 = mul(fsum(mul(dy, xh), 1, ROW_DEPTH, keepdim=True), invD).map(lambda u: u.expand(M, D))
    r = mul(sub(sub(dy, m1), mul(xh, m2)), col(rstd))
    if dres is not None:
        r = add(exact(dres), r)
    res = {"dx": out(r)}
    grp = lambda v: v.map(lambda u: u.reshape(G, rows_per_mod, D))  # noqa: E731
    depth = -(-rows_per_mod // 8) + 8  # rows of a wave in order, then the 8 waves in order
    a1 = fsum(grp(d), 1, depth)
    a2 = fsum(grp(mul(d, xh)), 1, depth)
    gx = lambda u: exact(u).map(lambda v: v[None].expand(G, D))  # noqa: E731
    if w is not None:
        res["dscale"] = out(add(mul(gx(w), a2), mul(gx(b), a1)))
    else:
        res["dscale"] = out(a2)  # 1.0f * a2 + 0.f * a1
    res["dshift"] = out(a1)
    if want_dwb:
        s1 = add(const(1.0, a1), exact(scale))
        res["dwb"] = out(V(torch.stack([mul(s1, a2).ref, mul(s1, a1).ref], 1), torch.stack([mul(s1, a2).err, mul(s1, a1).err], 1)))
    if gate_t is not None:
        res["dt"] = out(mul(r, exact(_rows_mod(gate, rows_per_mod, M))))
        res["dgate"] = out(fsum(grp(mul(r, exact(gate_t))), 1, depth))
    return res


# ------------------------------------------------------------------------------------------------------------------ QK-RMSNorm + RoPE
def rope_tables(rows: int, rot: int, gen, device):
    """cos / sin f32 [rows, rot / 2] of random angles (any table is a valid operand)"""
    ang = 6.0 * torch.rand(rows, max(rot // 2, 1), generator=gen, device=device)
    return ang.cos().float().contiguous(), ang.sin().float().contiguous()


def _rope_cs(cs, sn, tok_rows, H, dh, rot):
    """per-channel cos / sin [M, D] of the pair a channel belongs to, and the mask of rotated channels"""
    M = tok_rows.shape[0]
    on = (torch.arange(dh, device=tok_rows.device) < rot)
    pair = (torch.arange(dh, device=tok_rows.device) // 2).clamp_max(max(rot // 2 - 1, 0))
    if rot == 0:
        z = torch.zeros(M, H * dh, dtype=torch.float64, device=tok_rows.device)
        return z + 1.0, z, on.repeat(H)[None].expand(M, -1)
    c = cs.double()[tok_rows][:, pair].repeat(1, H)
    s = sn.double()[tok_rows][:, pair].repeat(1, H)
    return c, s, on.repeat(H)[None].expand(M, -1)


def _swap_pairs(t):
    """[.., D] -> the partner of every channel inside its (even, odd) pair"""
    return t.reshape(*t.shape[:-1], -1, 2).flip(-1).reshape(t.shape)


def _rotate(y: V, c, s, on, inverse: bool) -> V:
    """interleaved pairs: (a, b) -> (a c - b s, a s + b c); inverse: the transpose"""
    D = y.ref.shape[-1]
    even = (torch.arange(D, device=y.ref.device) % 2 == 0)[None]
    sign = torch.where(even, -1.0, 1.0).double() * (-1.0 if inverse else 1.0)
    p = y.map(_swap_pairs)
    rot = add(mul(y, V(c)), mul(p, V(s * sign)))  # two products and one sum (or an fma)
    return V(torch.where(on, rot.ref, y.ref), torch.where(on, rot.err, y.err))


def qk_fwd_ref(qkv, sq, sk, cs, sn, tok_rows, H, dh, rot, eps):
    """qkv [M, >= 2 D] (the logical columns); -> qk [M, 2 D], rrms [M, 2]"""
    M, D = qkv.shape[0], H * dh
    c, s, on = _rope_cs(cs, sn, tok_rows, H, dh, rot)
    qs, rs = [], []
    for part, scl in ((0, sq), (1, sk)):
        v = exact(qkv[:, part * D:(part + 1) * D])
        invD = _invn(D, V(v.ref[:, :1]))
        ms = mul(fsum(mul(v, v), 1, ROW_DEPTH, keepdim=True), invD)
        r = rcp(sqrt_(add(ms, const(f32c(eps), ms))))
        y = mul(mul(v, r.map(lambda u: u.expand(M, D))), exact(scl).map(lambda u: u[None].expand(M, D)))
        qs.append(_rotate(y, c, s, on, False))
        rs.append(r)
    return {"qk": (torch.cat([q.ref for q in qs], 1), torch.cat([q.err for q in qs], 1)),
            "rrms": (torch.cat([r.ref for r in rs], 1), torch.cat([r.err for r in rs], 1))}


def qk_bwd_ref(dqk, qkv, sq, sk, cs, sn, tok_rows, rrms, B, N, H, dh, rot):
    """from the f32 rrms as given; -> dqk_in [M, 2 D] (the q / k columns of dqkv), dscale [B, 2, D]"""
    M, D = qkv.shape[0], H * dh
    c, s, on = _rope_cs(cs, sn, tok_rows, H, dh, rot)
    dxs, dss = [], []
    depth = -(-N // 4) + 2  # tokens of a wave in order, then (w0 + w1) + (w2 + w3)
    for part, scl in ((0, sq), (1, sk)):
        g = _rotate(exact(dqk[:, part * D:(part + 1) * D]), c, s, on, True)
        x = exact(qkv[:, part * D:(part + 1) * D])
        r = exact(rrms[:, part]).map(lambda u: u[:, None].expand(M, D))
        dss.append(fsum(mul(mul(g, x), r).map(lambda u: u.reshape(B, N, D)), 1, depth))
        gx = mul(g, exact(scl).map(lambda u: u[None].expand(M, D)))
        invD = _invn(D, V(x.ref[:, :1]))
        m = mul(fsum(mul(gx, x), 1, ROW_DEPTH, keepdim=True), invD)
        r1 = V(r.ref[:, :1], r.err[:, :1])
        k = mul(mul(r1, r1), m).map(lambda u: u.expand(M, D))
        dxs.append(mul(r, sub(gx, mul(x, k))))
    return {"dqk_in": (torch.cat([v.ref for v in dxs], 1), torch.cat([v.err for v in dxs], 1)),
            "dscale": (torch.stack([v.ref for v in dss], 1), torch.stack([v.err for v in dss], 1))}


# ------------------------------------------------------------------------------------------------------------------ softmax
def softmax_depth(cols: int, vec: bool) -> int:
    """vec: <= 16 float4 chunks per lane, 2 inside a chunk, 6 tree levels; any: ceil(cols / 64) per lane + 6"""
    return (-(-cols // 256) + 2 + 6) if vec else (-(-cols // 64) + 6)


def softmax_v(s: V, depth: int) -> V:
    """over the last dimension; the subtracted maximum is whatever f32 value the kernel took (softmax is shift-invariant): exact"""
    mx = s.ref.max(-1, keepdim=True).values
    dead = torch.isinf(mx) & (mx < 0)  # every key masked: the keymask kernel writes zeros
    z = rnd(V(torch.where(torch.isinf(s.ref), s.ref, s.ref - torch.where(dead, torch.zeros_like(mx), mx)), s.err))
    z = V(z.ref, torch.where(torch.isinf(z.ref), torch.zeros_like(z.err), z.err))
    e = exp_(z)
    tot = fsum(e, -1, depth, keepdim=True)
    p = mul(e, rcp(tot).map(lambda u: u.expand_as(e.ref)))
    zero = torch.zeros_like(p.ref)
    return V(torch.where(dead, zero, p.ref), torch.where(dead, zero, p.err))


def softmax_fwd_ref(s, vec: bool, bias=None):
    sv = exact(s)
    if bias is not None:
        sv = V(sv.ref + bias.double())  # (+ 0 and + -inf are exact)
    return {"p": out(softmax_v(sv, softmax_depth(s.shape[-1], vec)))}


def softmax_bwd_v(p: V, dp: V, depth: int) -> V:
    dot = fsum(mul(p, dp), -1, depth, keepdim=True)
    return mul(p, sub(dp, dot.map(lambda u: u.expand_as(p.ref))))


def softmax_bwd_ref(p, dp, vec: bool):
    return {"ds": out(softmax_bwd_v(exact(p), exact(dp), softmax_depth(p.shape[-1], vec)))}


# ------------------------------------------------------------------------------------------------------------------ attention composites
def _heads(t, B, n, H, dh):
    """[B n, H dh] rows -> [B, H, n, dh]"""
    return t.reshape(B, n, H, dh).permute(0, 2, 1, 3)


def attn_ref(q, k, v, dout, B, Nq, L, H, dh, key_bias=None):
    """ops.f32_attn_fwd / _bwd (Nq == L, no bias) and ops.f32_xattn_fwd / _bwd as compositions of the GEMM and softmax bounds;
    -> out, probs, dq, dk, dv.  The backward GEMMs read the f32 probabilities and dS the kernels stored: their errors carry through."""
    hq = lambda t: exact(t).map(lambda u: _heads(u, B, Nq, H, dh))  # noqa: E731
    hk = lambda t: exact(t).map(lambda u: _heads(u, B, L, H, dh))  # noqa: E731
    tr = lambda a: a.map(lambda u: u.transpose(-1, -2))  # noqa: E731
    back = lambda a, n: a.map(lambda u: u.permute(0, 2, 1, 3).reshape(B * n, H * dh))  # noqa: E731
    Q, K_, Vv, dO = hq(q), hk(k), hk(v), hq(dout)
    alpha = const(f32c(float(dh) ** -0.5), V(Q.ref[..., :1, :1]))
    al = lambda a: mul(a, alpha.map(lambda u: u.expand_as(a.ref)))  # noqa: E731
    S = al(matmul(Q, tr(K_)))
    any_form = key_bias is not None or L % 4 != 0 or L > 4096
    if key_bias is not None:
        kb = exact(key_bias).map(lambda u: u[:, None, None, :].expand_as(S.ref))
        S = V(S.ref + kb.ref, S.err)  # (+ 0 and + -inf are exact)
        S = V(S.ref, torch.where(torch.isfinite(S.ref), S.err, torch.zeros_like(S.err)))
    depth = softmax_depth(L, not any_form)
    P = softmax_v(S, depth)
    O = matmul(P, Vv)
    dP = matmul(dO, tr(Vv))
    dV = matmul(tr(P), dO)
    dS = softmax_bwd_v(P, dP, softmax_depth(L, L % 4 == 0 and L <= 4096))
    dQ = al(matmul(dS, K_))
    dK = al(matmul(tr(dS), Q))
    return {"out": out(back(O, Nq)), "probs": out(P), "dq": out(back(dQ, Nq)), "dk": out(back(dK, L)), "dv": out(back(dV, L))}


# ------------------------------------------------------------------------------------------------------------------ token routing, gates, DDT
def scatter_add_ref(src, idx, dst0, B, N, k):
    """dst[b, idx[b, j]] += src[b, j] (idx unique per sample): one rounding; untouched rows keep their bits (err 0)"""
    D = src.shape[1]
    s = exact(src).map(lambda u: u.reshape(B, k, D))
    d0 = exact(dst0).map(lambda u: u.reshape(B, N, D))
    ii = idx.reshape(B, k).long()[:, :, None].expand(B, k, D)
    upd = torch.zeros_like(d0.ref).scatter(1, ii, s.ref)
    hit = torch.zeros_like(d0.ref, dtype=torch.bool).scatter(1, ii, torch.ones_like(s.ref, dtype=torch.bool))
    r = rnd(V(d0.ref + upd))
    return {"dst": ((r.ref).reshape(B * N, D), torch.where(hit, r.err, torch.zeros_like(r.err)).reshape(B * N, D))}


def restore_ref(xd, inv, mask, B, N, k):
    D = xd.shape[1]
    j = inv.reshape(B, N).long()
    g = xd.reshape(B, k, D).gather(1, j.clamp_min(0)[:, :, None].expand(B, N, D))
    return {"out": bits(torch.where((j >= 0)[:, :, None], g, mask[None, None, :]).reshape(B * N, D))}


def colsum_ref(x, sel, slabs):
    R, C = x.shape
    rps = -(-R // slabs)
    xm = torch.where((sel < 0)[:, None], x.double(), torch.zeros(1, dtype=torch.float64, device=x.device))
    pad = torch.zeros(slabs * rps - R, C, dtype=torch.float64, device=x.device)
    v = exact(torch.cat([xm, pad], 0)).map(lambda u: u.reshape(slabs, rps, C))
    return {"part": out(fsum(v, 1, -(-rps // 4) + 2))}


def gated_residual_ref(x, t, gate, rows_per_mod):
    M = x.shape[0]
    return {"out": out(add(exact(x), mul(exact(_rows_mod(gate, rows_per_mod, M)), exact(t))))}


def gate_bwd_ref(dout, t, gate, rows_per_mod):
    M, D = dout.shape
    G = M // rows_per_mod
    d = exact(dout)
    dg = fsum(mul(d, exact(t)).map(lambda u: u.reshape(G, rows_per_mod, D)), 1, -(-rows_per_mod // 8) + 3)
    return {"dt": out(mul(d, exact(_rows_mod(gate, rows_per_mod, M)))), "dgate": out(dg)}


def ddt_fwd_ref(enc, temb, N):
    u = add(exact(enc), exact(temb.repeat_interleave(N, 0)))
    return {"out": out(silu_(silu_(u)))}


def ddt_bwd_ref(dsz, enc, temb, N):
    M, D = enc.shape
    B = M // N
    u = add(exact(enc), exact(temb.repeat_interleave(N, 0)))
    de = mul(mul(exact(dsz), dsilu_(silu_(u))), dsilu_(u))
    return {"denc": out(de), "dtemb": out(fsum(de.map(lambda t: t.reshape(B, N, D)), 1, -(-N // 8) + 3))}


# ------------------------------------------------------------------------------------------------------------------ elementwise
INV_SQRT2 = 0.70710678118654752
INV_SQRT2PI = 0.39894228040143268


def _cst(x: float, like: V) -> V:
    """a decimal constant of the source: its f32 value against the real number it stands for"""
    return V(torch.full_like(like.ref, x), torch.full_like(like.ref, abs(f32c(x) - x)))


def geglu_fwd_ref(u, F):
    a, g = exact(u[:, :F]), exact(u[:, F:2 * F])
    cdf2 = add(const(1.0, g), erf_(mul(g, _cst(INV_SQRT2, g))))
    return {"h": out(mul(a, mul(mul(const(0.5, g), g), cdf2)))}


def geglu_bwd_ref(dh, u, F):
    a, g, d = exact(u[:, :F]), exact(u[:, F:2 * F]), exact(dh)
    cdf = scale2(add(const(1.0, g), erf_(mul(g, _cst(INV_SQRT2, g)))), 0.5)
    da = mul(mul(d, g), cdf)
    pdf = exp_(mul(scale2(neg(g), 0.5), g))
    dg = mul(mul(d, a), add(cdf, mul(mul(g, _cst(INV_SQRT2PI, g)), pdf)))
    return {"du": (torch.cat([da.ref, dg.ref], 1), torch.cat([da.err, dg.err], 1))}


def swiglu_fwd_ref(u, F):
    return {"h": out(mul(silu_(exact(u[:, :F])), exact(u[:, F:2 * F])))}


def swiglu_bwd_ref(dh, u, F):
    x1, x3, g = exact(u[:, :F]), exact(u[:, F:2 * F]), exact(dh)
    d1, d3 = mul(mul(g, x3), dsilu_(x1)), mul(g, silu_(x1))
    return {"du": (torch.cat([d1.ref, d3.ref], 1), torch.cat([d1.err, d3.err], 1))}


def add_ref(a, b):
    return {"out": out(add(exact(a), exact(b)))}


def silu_bwd_ref(dy, pre):
    return {"dx": out(mul(exact(dy), dsilu_(exact(pre))))}


def patchify_ref(x, p, ld, order_cpp: bool):
    B, C, H, W = x.shape
    gh, gw = H // p, W // p
    t = x.reshape(B, C, gh, p, gw, p)
    t = t.permute(0, 2, 4, 1, 3, 5) if order_cpp else t.permute(0, 2, 4, 3, 5, 1)
    t = t.reshape(B * gh * gw, C * p * p)
    return {"tok": bits(torch.nn.functional.pad(t, (0, ld - C * p * p)))}


def timestep_ref(t, dim, max_period):
    """[cos(t f_k) | sin(t f_k)], f_k = exp(-ln(P) k / half); an odd dim ends in a zero column"""
    B, half = t.shape[0], dim // 2
    k = torch.arange(half, dtype=torch.float64, device=t.device)[None].expand(B, half)
    nlp = -math.log(max_period)
    kv = V(k)
    # -logf(P) on the host: 1 ulp; (float)k * nlp rounded; / (float)half one division
    z = div(mul(kv, V(torch.full_like(k, nlp), torch.full_like(k, 2 * U * abs(nlp)))), const(float(half), kv))
    f = exp_(z)
    f = V(f.ref, torch.where(k == 0, torch.zeros_like(f.err), f.err))  # expf(0) = 1
    a = mul(exact(t).map(lambda u: u[:, None].expand(B, half)), f)
    c, s = cos_(a), sin_(a)
    pad = torch.zeros(B, dim - 2 * half, dtype=torch.float64, device=t.device)
    return {"emb": (torch.cat([c.ref, s.ref, pad], 1), torch.cat([c.err, s.err, pad], 1))}


def cond_fwd_ref(e, table, idx):
    v = exact(e) if table is None else add(exact(e), exact(table[idx]))
    return {"emb": out(v), "act": out(silu_(v))}


def cond_bwd_ref(dact, emb, idx, dtable0):
    """demb = dact silu'(emb); dtable[idx[b]] += demb[b] in batch order"""
    g = mul(exact(dact), dsilu_(exact(emb)))
    res = {"demb": out(g)}
    if dtable0 is not None:
        n_cls, E = dtable0.shape
        B = dact.shape[0]
        onehot = torch.nn.functional.one_hot(idx, n_cls).double()  # [B, n_cls]
        cnt = onehot.sum(0)  # additions a table row takes
        r = dtable0.double() + onehot.t() @ g.ref
        mag = dtable0.double().abs() + onehot.t() @ g.mag
        res["dtable"] = (r, onehot.t() @ g.err + ACC_C * cnt[:, None] * U * mag + TINY * (cnt[:, None] > 0))
    return res


# ------------------------------------------------------------------------------------------------------------------ UNet
def _taps(x4):
    """x4 [B, H, W, C] -> [B, H, W, C, 9]: tap = 3 ky + kx reads pixel (y + ky - 1, x + kx - 1), zero outside"""
    B, H, W, C = x4.shape
    xp = torch.nn.functional.pad(x4, (0, 0, 1, 1, 1, 1))
    return torch.stack([xp[:, ky:ky + H, kx:kx + W, :] for ky in range(3) for kx in range(3)], -1)


def im2col_ref(x, B, H, W, C):
    return {"cols": bits(_taps(x.reshape(B, H, W, C)).reshape(B * H * W, C * 9))}


def col2im_ref(dcols, B, H, W, C):
    """the adjoint: dx[p', c] = sum_tap dcols[p' - shift(tap), c, tap], at most 9 terms in tap order"""
    d = dcols.double().reshape(B, H, W, C, 9)
    dp = torch.nn.functional.pad(d, (0, 0, 0, 0, 1, 1, 1, 1))
    terms = torch.stack([dp[:, 2 - ky:2 - ky + H, 2 - kx:2 - kx + W, :, 3 * ky + kx] for ky in range(3) for kx in range(3)], -1)
    return {"dx": out(V(*fsum(V(terms), -1, 9).pair()).map(lambda u: u.reshape(B * H * W, C)))}


def gn_stats_ref(x, B, HW, C, G, eps):
    """two passes over HW C/G elements: 256 threads in order, the wave tree, four waves"""
    cg = C // G
    n = HW * cg
    depth = -(-n // 256) + 6 + 2
    xg = exact(x).map(lambda u: u.reshape(B, HW, G, cg).permute(0, 2, 1, 3).reshape(B, G, n))
    nf = const(float(n), V(xg.ref[..., :1]))
    mu = div(fsum(xg, 2, depth, keepdim=True), nf)
    d_own = rnd(V(xg.ref - mu.ref))
    var = div(fsum(mul(d_own, d_own), 2, depth, keepdim=True), nf)
    var = V(var.ref, var.err + mu.err.square())
    rs = rcp(sqrt_(add(var, const(f32c(eps), var))))
    return {"stats": (torch.stack([mu.ref[..., 0], rs.ref[..., 0]], -1), torch.stack([mu.err[..., 0], rs.err[..., 0]], -1))}


def _gn_pre(x, stats, w, b, fs, fh, B, HW, C, G):
    """-> xh, y, z (V [B, HW, C]) and f1 [B, 1, C] from the f32 statistics as given"""
    cg = C // G
    e3 = lambda u: u.expand(B, HW, C)  # noqa: E731
    ch = lambda t: exact(t).map(lambda u: e3(u.repeat_interleave(cg, 1)[:, None, :]))  # noqa: E731
    xv = exact(x).map(lambda u: u.reshape(B, HW, C))
    xh = mul(sub(xv, ch(stats[..., 0])), ch(stats[..., 1]))
    wv, bv = (exact(t).map(lambda u: e3(u[None, None, :])) for t in (w, b))
    y = add(mul(xh, wv), bv)
    if fs is not None:
        f1 = add(const(1.0, xv), exact(fs).map(lambda u: e3(u[:, None, :])))
        z = add(mul(y, f1), exact(fh).map(lambda u: e3(u[:, None, :])))
    else:
        f1, z = const(1.0, xv), y
    return xh, y, z, f1, wv


def gn_apply_ref(x, stats, w, b, fs, fh, silu, B, HW, C, G):
    _, _, z, _, _ = _gn_pre(x, stats, w, b, fs, fh, B, HW, C, G)
    return {"out": out((silu_(z) if silu else z).map(lambda u: u.reshape(B * HW, C)))}


def gn_bwd_ref(dout, x, stats, w, b, fs, fh, silu, dres, B, HW, C, G):
    """-> dx [B HW, C], dw / db partials [B, C] (+ dfs, dfh [B, C])"""
    cg = C // G
    R = max(256 // cg, 1)
    xh, y, z, f1, wv = _gn_pre(x, stats, w, b, fs, fh, B, HW, C, G)
    d = exact(dout).map(lambda u: u.reshape(B, HW, C))
    dz = mul(d, dsilu_(z)) if silu else d
    dy = mul(dz, f1) if fs is not None else dz
    dxh = mul(dy, wv)
    d_ch = -(-HW // R) + R  # a pixel lane's pixels in order, then the R lanes in order
    d_gr = -(-HW // R) + 6 + 2  # ... then the wave tree and the four waves
    grp = lambda v: v.map(lambda u: u.reshape(B, HW, G, cg).permute(0, 2, 1, 3).reshape(B, G, HW * cg))  # noqa: E731
    nf = V(torch.full((B, G, 1), float(HW) * float(cg), dtype=torch.float64, device=x.device))
    m1 = div(fsum(grp(dxh), 2, d_gr, keepdim=True), nf)
    m2 = div(fsum(grp(mul(dxh, xh)), 2, d_gr, keepdim=True), nf)
    chn = lambda v: v.map(lambda u: u[..., 0].repeat_interleave(cg, 1)[:, None, :].expand(B, HW, C))  # noqa: E731
    rsc = exact(stats[..., 1]).map(lambda u: u.repeat_interleave(cg, 1)[:, None, :].expand(B, HW, C))
    dx = mul(rsc, sub(sub(dxh, chn(m1)), mul(xh, chn(m2))))
    if dres is not None:
        dx = add(exact(dres).map(lambda u: u.reshape(B, HW, C)), dx)
    res = {"dx": out(dx.map(lambda u: u.reshape(B * HW, C))), "dw": out(fsum(mul(dy, xh), 1, d_ch)), "db": out(fsum(dy, 1, d_ch))}
    if fs is not None:
        res["dfs"] = out(fsum(mul(dz, y), 1, d_ch))
        res["dfh"] = out(fsum(dz, 1, d_ch))
    return res


def resample_ref(x, B, Hs, Ws, C, scale, mode):
    """mode 0 reduce: scale ((a + b) + (c + d)); 1 expand: scale x (one rounding; exact for a power of two); 2 pick, 3 stuff: bits"""
    if mode == 0:
        t = exact(x).map(lambda u: u.reshape(B, Hs, 2, Ws, 2, C))
        g = lambda i, j: t.map(lambda u: u[:, :, i, :, j, :])  # noqa: E731
        v = mul(const(f32c(scale), g(0, 0)), add(add(g(0, 0), g(0, 1)), add(g(1, 0), g(1, 1))))
        return {"out": out(v.map(lambda u: u.reshape(B * Hs * Ws, C)))}
    if mode == 1:
        t = exact(x).map(lambda u: u.reshape(B, Hs, 1, Ws, 1, C).expand(B, Hs, 2, Ws, 2, C).reshape(B * 4 * Hs * Ws, C))
        return {"out": out(mul(const(f32c(scale), t), t))}
    if mode == 2:
        return {"out": bits(x.reshape(B, Hs, 2, Ws, 2, C)[:, :, 0, :, 0, :].reshape(B * Hs * Ws, C))}
    o = torch.zeros(B, Hs, 2, Ws, 2, C, dtype=x.dtype, device=x.device)
    o[:, :, 0, :, 0, :] = x.reshape(B, Hs, Ws, C)
    return {"out": bits(o.reshape(B * 4 * Hs * Ws, C))}


def rowbias_add_ref(x, e, B, HW, C):
    return {"out": out(add(exact(x).map(lambda u: u.reshape(B, HW, C)), exact(e).map(lambda u: u[:, None, :].expand(B, HW, C)))
                       .map(lambda u: u.reshape(B * HW, C)))}


def rowbias_bwd_ref(dy, B, HW, C):
    return {"de": out(fsum(exact(dy).map(lambda u: u.reshape(B, HW, C)), 1, HW))}


# ------------------------------------------------------------------------------------------------------------------ judging
def worst_ratio(got, ref, bound) -> float:
    """max |got - ref| / bound; 0 / 0 counts as 0, NaN and a miss of a zero bound as inf"""
    d = (got.to(ref.device).double() - ref).abs()
    r = torch.where(d == 0, torch.zeros_like(d), d / bound)
    return float(torch.nan_to_num(r, nan=float("inf")).max()) if r.numel() else 0.0


def same_bits(a, b) -> bool:
    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32).to(a.device)))


def judge(got: dict, ref: dict) -> dict:
    """-> {output: worst |diff| / bound, or 0.0 / inf for a bit-compare}; every bound must be finite"""
    res = {}
    for name, (r, bound) in ref.items():
        g = got[name]
        assert tuple(g.shape) == tuple(r.shape), (name, tuple(g.shape), tuple(r.shape))
        if bound is None:
            res[name] = 0.0 if same_bits(g, r) else float("inf")
        else:
            assert bool(torch.isfinite(bound).all()), f"{name}: a bound is not finite"
            res[name] = worst_ratio(g, r, bound)
    return res


# ------------------------------------------------------------------------------------------------------------------ inputs
def row_input(cls: str, M: int, D: int, gen, device):
    """f32 [M, D] of one input class.  scaled: per-column scale in [0.5, 2.5] and offset 1.5 N(0, 1); offset32: row mean at 32 x the
    row std (signs alternate); const: as scaled with row 1 % M constant (true variance 0: the variance term is eps alone)"""
    n = lambda *s: torch.randn(s, generator=gen, device=device)  # noqa: E731
    if cls == "offset32":
        sd = 0.5 + 1.5 * torch.rand(M, 1, generator=gen, device=device)
        sign = (1.0 - 2.0 * (torch.arange(M, device=device) % 2))[:, None]
        return n(M, D) * sd + 32.0 * sd * sign
    x = n(M, D) * (0.5 + 2.0 * torch.rand(1, D, generator=gen, device=device)) + 1.5 * n(1, D)
    if cls == "const":
        x[1 % M] = 2.71875
    else:
        assert cls == "scaled", cls
    return x


ROW_CLASSES = ("scaled", "offset32", "const")


# ------------------------------------------------------------------------------------------------------------------ coverage
# every dl_f32_* entry point of include/diffulab_hip.h -> the tests of tests/test_f32_paths_gpu.py that call it
COVERAGE = {
    "dl_f32_gemm": ["test_gemm", "test_gemm_batched_pre_out", "test_attention_composites"],
    "dl_f32_ln_modulate_fwd": ["test_ln_modulate", "test_ln_modulate_refuses_wide_rows"],
    "dl_f32_ln_modulate_bwd": ["test_ln_modulate", "test_ln_modulate_refuses_wide_rows"],
    "dl_f32_qk_norm_rope_fwd": ["test_qk_norm_rope"],
    "dl_f32_qk_norm_rope_bwd": ["test_qk_norm_rope"],
    "dl_f32_scatter_tokens_add": ["test_token_routing"],
    "dl_f32_restore_tokens": ["test_token_routing"],
    "dl_f32_masked_colsum_partials": ["test_masked_colsum"],
    "dl_f32_gated_residual_fwd": ["test_gates_and_ddt"],
    "dl_f32_gate_bwd": ["test_gates_and_ddt"],
    "dl_f32_ddt_cond_fwd": ["test_gates_and_ddt"],
    "dl_f32_ddt_cond_bwd": ["test_gates_and_ddt"],
    "dl_f32_softmax_fwd": ["test_softmax", "test_attention_composites"],
    "dl_f32_softmax_bwd": ["test_softmax", "test_attention_composites"],
    "dl_f32_softmax_keymask_fwd": ["test_softmax_keymask", "test_attention_composites"],
    "dl_f32_geglu_fwd": ["test_elementwise"],
    "dl_f32_geglu_bwd": ["test_elementwise"],
    "dl_f32_swiglu_fwd": ["test_elementwise"],
    "dl_f32_swiglu_bwd": ["test_elementwise"],
    "dl_f32_add": ["test_elementwise"],
    "dl_f32_silu_bwd": ["test_elementwise"],
    "dl_f32_patchify": ["test_patchify"],
    "dl_f32_timestep_embedding": ["test_timestep_embedding"],
    "dl_f32_cond_combine_fwd": ["test_cond_combine"],
    "dl_f32_cond_combine_bwd": ["test_cond_combine"],
    "dl_f32_im2col3x3": ["test_unet_data_movement"],
    "dl_f32_col2im3x3": ["test_unet_data_movement"],
    "dl_f32_gn_stats": ["test_groupnorm"],
    "dl_f32_gn_apply_fwd": ["test_groupnorm"],
    "dl_f32_gn_bwd": ["test_groupnorm", "test_groupnorm_bwd_refuses_wide_groups"],
    "dl_f32_resample2x2": ["test_unet_data_movement"],
    "dl_f32_nchw_to_nhwc": ["test_unet_data_movement"],
    "dl_f32_nhwc_to_nchw": ["test_unet_data_movement"],
    "dl_f32_copy2d": ["test_unet_data_movement"],
    "dl_f32_rowbias_add": ["test_unet_data_movement"],
    "dl_f32_rowbias_bwd": ["test_unet_data_movement"],
}
