"""fp64 references and element-wise error bounds for the softmax-attention kernels (imported by the test modules; not a conftest).

The GEMM-family bounds live in elementwise_bounds.py; this module reuses its constants (U32, ACC_C), its bf16 / f32 store terms and
its poisoned buffers.  Every function takes the kernel's bf16 / f32 operands, returns (reference, bound) pairs in fp64 on the
operands' device and works on G = B * H independent heads: q [G, Nq, dh], k / v [G, Nk, dh], bias [G, Nk] (0 = keep, -inf = masked).

What the DiT kernels compute (attn_fwd_k / attn_bwd_k in csrc/attention.hip; the tiled, fused-norm and long forms follow it), with
U = 2^-24 and C = 2:
  forward   s2 = fl(acc c) (+ fl(bias log2 e)), acc = the f32 MFMA sum of 64 products, c = fl(scale log2 e); per 64-key block the
            running maximum m, p = v_exp_f32(s2 - m), l += sum of the f32 p, o = o alpha + V^T bf16(p); out = bf16(o / l),
            lse = (m + log2 l) ln 2
  backward  p = v_exp_f32(fl(acc c) + bias log2 e - fl(lse log2 e)), dP = f32 MFMA sum of 64 products, delta = f32 sum of out dO,
            dS = p (dP - delta); dv = bf16(sum bf16(p) dO), dq = bf16(scale sum bf16(dS) k), dk = bf16(scale sum bf16(dS) q)
The backward's reference is a function of the backward's actual inputs -- the forward's own bf16 `out` and f32 `lse` included --
because that is what the kernel computes; the forward is bounded against fp64 on its own, so the chain covers the true gradient.
A masked key has probability exactly 0 in the reference and in the kernels (exp2(-inf) = 0): its dk / dv rows are compared for
equality by the tests, and its entries are excluded from every exponent-error term (0 * inf).

The UNet kernels (attn_small_* / attn_cross_*, MFMA forms in csrc/attention.hip, VALU forms in csrc/unet.hip) normalise the
probabilities in f32, save them (`probs`, a checked output) and read them back in the backward: probs_* below.  The MFMA forms round
P and dS to bf16 for their products (bf16_p = True: rnd_bf16, half a bf16 ulp of each element), the VALU forms multiply in f32
(bf16_p = False).

The rounding of p (and dS) to bf16 is bounded by half a bf16 ulp of each element (rnd_bf16), not by a flat 2^-9 p: bf16 keeps 8
significand bits, so rounding to nearest errs by up to 2^(e - 9) for p in [2^(e - 1), 2^e), which is 2^-9 p only at the top of a
binade and 2^-8 p at its bottom.  With the flat 2^-9 p the faithful emulation of the host test leaves the dq / dk / dv bounds on
the peaked input (1.1 to 1.3 times the bound); with the exact half ulp it stays inside and both truncation mutants are still rejected.

Error classes these bounds cannot see, by construction (tests/test_attention_bounds_host.py demonstrates each):
  * `lse` off by one f32 ulp of 8.0 (2^-20): the kernel's own log2 l (v_log_f32, 1 ulp of a value up to 11) and the 64-term f32 score
    sums behind m are allowed more than that, so no sound bound rejects it.  What does see a form whose lse drifts from the others
    is the bit-for-bit comparison of the forms: test_attn_paths_gpu.py::test_attn_path (inference against training form, every
    case twice) and test_row_gemm_gpu.py::test_pipelined_attention_forward_equals_the_chain_form_bit_for_bit.
"""

from __future__ import annotations

import math

import torch

import elementwise_bounds as eb

U = eb.U32
C = eb.ACC_C
TINY = 2.0**-126  # v_exp_f32 flushes results below the smallest normal f32 to zero
SCORE_K = 64  # contraction length of the DiT score / dP products (head_dim)
MAX_ELEMS = 1 << 23  # fp64 score-matrix elements per slice of heads (64 MiB per temporary)


def f32(x: float) -> float:
    """the f32 value a float argument of the C ABI arrives as"""
    return float(torch.tensor(x, dtype=torch.float32))


def rnd_bf16(x, on: bool = True):
    """the error of rounding a value of magnitude x (>= 0) to the nearest bf16: half an ulp, 2^(e - 9) for x in [2^(e - 1), 2^e) --
    between 2^-9 x at the top of a binade and 2^-8 x at its bottom (a flat 2^-9 x is not a bound: p = 0.501 rounds by up to 2^-10);
    0 for x = 0 and for the f32 VALU forms (on = False)"""
    if not on:
        return torch.zeros_like(x)
    return torch.where(x > 0, eb.half_ulp(x, 8), torch.zeros_like(x))


def _heads_per_slice(nq: int, nk: int) -> int:
    return max(1, MAX_ELEMS // (nq * nk))


def _sliced(fn, G: int, nq: int, nk: int, *tensors):
    """fn over slices of heads, so that no fp64 [g, Nq, Nk] temporary exceeds MAX_ELEMS elements (2048 x 2048: two heads at a time)"""
    step = _heads_per_slice(nq, nk)
    parts = [fn(*[None if t is None else t[g:g + step] for t in tensors]) for g in range(0, G, step)]
    return tuple(torch.cat([p[i] for p in parts]) for i in range(len(parts[0])))


def _scores(q, k, scale, bias):
    """fp64 scores S, the magnitude sum A = (|q| |k|^T) scale, the keep mask, |bias| with masked entries as 0"""
    Q, K = q.double(), k.double()
    S = Q @ K.transpose(-1, -2) * scale
    A = Q.abs() @ K.abs().transpose(-1, -2) * scale
    if bias is None:
        return S, A, None, 0.0
    b = bias.double()[:, None, :]
    keep = ~torch.isinf(b)
    return S + b, A, keep, torch.where(keep, b.abs(), torch.zeros_like(b))


# ------------------------------------------------------------------------------------------------------------------ DiT family, forward
def _fwd_slice(q, k, v, bias, scale, bf16_p, score_k):
    S, A, keep, babs = _scores(q, k, scale, bias)
    Nk = k.shape[1]
    lse = torch.logsumexp(S, dim=-1)
    P = torch.exp(S - lse[..., None])
    V = v.double()
    Amax = A.max(dim=-1, keepdim=True).values + (babs.max() if bias is not None else 0.0)
    # relative error of one f32 p against exp(S - max), as an error of its exponent in natural units:
    eps = (C * score_k * U * A  # the f32 MFMA accumulation of the score, score_k products
           + 4 * U * A  # c = fl(scale * fl(log2 e)) (2 roundings), the product acc * c, the addition of the bias
           + 3 * U * babs  # fl(bias * fl(log2 e)) and its share of the sum's rounding
           + U * (A + Amax)  # the subtraction of the running maximum
           + 2 * U)  # v_exp_f32: 1 ulp
    eps = torch.expm1(eps)
    if keep is not None:
        eps = torch.where(keep, eps, torch.zeros_like(eps))  # masked: p = 0 exactly on both sides
    PV = P @ V.abs()
    ebar = (P * eps).sum(-1, keepdim=True)  # relative error of the row sum l (the denominator)
    ref = P @ V
    err = rnd_bf16(P * (1 + eps), bf16_p) @ V.abs()  # p rounded to bf16 for the PV MFMA (l is summed from the unrounded p)
    err = err + (P * eps) @ V.abs()  # exponent error through the numerator
    err = err + ebar / (1 - ebar) * PV  # ... and through the denominator
    err = err + C * Nk * U * PV  # f32 accumulation of the numerator over Nk terms
    err = err + Nk * U * PV  # f32 accumulation of l over Nk terms
    err = err + (2 * (Nk // 64 + 1) + 4) * U * PV  # o * alpha and l * alpha once per 64-key block; 1 / l (1 ulp) and o * inv
    err = err + TINY * V.abs().sum(1, keepdim=True)  # p below 2^-126 flushed to zero
    bound = eb.store_bf16(ref, err)  # the bf16 store
    # lse = (m + log2 l) ln 2
    e_l = ebar.squeeze(-1)  # the exponent errors, weighted as they enter l
    e_l = e_l + (Nk + 2 * (Nk // 64 + 1)) * U  # f32 sum of l; l * alpha per block
    e_l = e_l + (2 * (Nk // 64 + 1) + 2 * Amax.squeeze(-1)) * U  # alpha = v_exp_f32(fl(m_old - m_new)): 1 ulp per block, and the
    #                                                               roundings of the differences, which telescope to <= 2 max|s|
    e_l = e_l + 2 * U * math.log2(max(Nk, 2)) * math.log(2.0)  # log2f(l): 1 ulp of a value <= log2 Nk
    e_l = e_l + 3 * U * (lse.abs() + e_l)  # the addition m + log2 l, fl(ln 2) and the product
    return ref, bound, lse, eb.store_f32(lse, e_l)


def attn_fwd(q, k, v, scale: float, bias=None, bf16_p: bool = True, score_k: int = SCORE_K):
    """(out, out_bound, lse, lse_bound): out [G, Nq, dh] against the kernel's bf16 `out`, lse [G, Nq] against its f32 `lse`"""
    G, Nq, Nk = q.shape[0], q.shape[1], k.shape[1]
    return _sliced(lambda a, b, c, d: _fwd_slice(a, b, c, d, scale, bf16_p, score_k), G, Nq, Nk, q, k, v, bias)


# ------------------------------------------------------------------------------------------------------------------ DiT family, backward
def _bwd_slice(q, k, v, do, out, lse, bias, scale, bf16_p, score_k):
    S, A, keep, babs = _scores(q, k, scale, bias)
    Nq, Nk = q.shape[1], k.shape[1]
    Q, K, V, DO, O, L = q.double(), k.double(), v.double(), do.double(), out.double(), lse.double()[..., None]
    P = torch.exp(S - L)
    # relative error of one f32 p against exp(S - lse), as an error of its exponent:
    eps = (C * score_k * U * A  # the f32 MFMA accumulation of the score
           + 4 * U * A  # c = fl(scale * fl(log2 e)), the product acc * c, the addition of the bias
           + 3 * U * babs  # fl(bias * fl(log2 e))
           + 2 * U * L.abs()  # lse2 = fl(lse * fl(log2 e))
           + U * (A + babs + L.abs())  # the subtraction of lse2
           + 2 * U)  # v_exp_f32: 1 ulp
    eps = torch.expm1(eps)
    if keep is not None:
        eps = torch.where(keep, eps, torch.zeros_like(eps))
    dP = DO @ V.transpose(-1, -2)
    delta = (O * DO).sum(-1, keepdim=True)
    e_dp = C * score_k * U * (DO.abs() @ V.abs().transpose(-1, -2))  # f32 MFMA accumulation of dP
    e_dl = C * score_k * U * (O.abs() * DO.abs()).sum(-1, keepdim=True)  # f32 accumulation of delta
    diff = dP - delta
    e_diff = e_dp + e_dl + U * (diff.abs() + e_dp + e_dl)  # one rounding of the difference
    dS = P * diff
    # |dS~ - dS| <= p e_diff (1 + eps) + |dS| (eps + U): the product p * diff rounds once
    e_ds = P * e_diff * (1 + eps) + dS.abs() * (eps + U)
    e_ds_r = e_ds + rnd_bf16(dS.abs() + e_ds, bf16_p)  # dS rounded to bf16 for the dq / dk MFMAs
    e_p_r = P * eps + rnd_bf16(P * (1 + eps), bf16_p)  # p rounded to bf16 for the dv MFMA
    DOa, Ka, Qa = DO.abs(), K.abs(), Q.abs()
    # dv = P^T dO
    dv = P.transpose(-1, -2) @ DO
    e_dv = e_p_r.transpose(-1, -2) @ DOa  # (half a bf16 ulp of p + eps p)^T |dO|
    e_dv = e_dv + C * Nq * U * (P.transpose(-1, -2) @ DOa)  # f32 accumulation over Nq queries
    e_dv = e_dv + TINY * DOa.sum(1, keepdim=True)  # p below 2^-126 flushed to zero
    # dq = scale dS k
    dq = scale * (dS @ K)
    e_dq = scale * (e_ds_r @ Ka)  # scale (half a bf16 ulp of dS + eps |dS|) |k| plus the dS-side f32 terms
    e_dq = e_dq + scale * C * Nk * U * (dS.abs() @ Ka)  # f32 accumulation over Nk keys
    e_dq = e_dq + U * (dq.abs() + e_dq)  # the multiplication by scale at the store
    # dk = scale dS^T q
    dk = scale * (dS.transpose(-1, -2) @ Q)
    e_dk = scale * (e_ds_r.transpose(-1, -2) @ Qa)
    e_dk = e_dk + scale * C * Nq * U * (dS.abs().transpose(-1, -2) @ Qa)  # f32 accumulation over Nq queries
    e_dk = e_dk + U * (dk.abs() + e_dk)  # the multiplication by scale at the store
    return dq, eb.store_bf16(dq, e_dq), dk, eb.store_bf16(dk, e_dk), dv, eb.store_bf16(dv, e_dv)


def attn_bwd(q, k, v, do, out, lse, scale: float, bias=None, bf16_p: bool = True, score_k: int = SCORE_K):
    """(dq, dq_bound, dk, dk_bound, dv, dv_bound) from the backward's own inputs: do / out [G, Nq, dh] (the forward's bf16 out),
    lse [G, Nq] (the forward's f32 lse)"""
    G, Nq, Nk = q.shape[0], q.shape[1], k.shape[1]
    return _sliced(lambda *a: _bwd_slice(*a, scale, bf16_p, score_k), G, Nq, Nk, q, k, v, do, out, lse, bias)


def attn_grad_fp64(q, k, v, do, scale: float, bias=None):
    """the true gradient (fp64 autograd of the bf16 operands), for the whole-chain relative-L2 check at the suite's older thresholds"""
    Q, K, V = (t.double().detach().requires_grad_(True) for t in (q, k, v))
    step = _heads_per_slice(q.shape[1], k.shape[1])
    for g in range(0, q.shape[0], step):
        s = Q[g:g + step] @ K[g:g + step].transpose(-1, -2) * scale
        if bias is not None:
            s = s + bias[g:g + step].double()[:, None, :]
        o = torch.softmax(s, dim=-1) @ V[g:g + step]
        o.backward(do[g:g + step].double())
    return Q.grad, K.grad, V.grad


# ------------------------------------------------------------------------------------------------------------------ UNet small / cross
def _probs_fwd_slice(q, k, v, bias, scale, bf16_p):
    S, A, keep, babs = _scores(q, k, scale, bias)
    dh, L = q.shape[2], k.shape[1]
    m = S.max(dim=-1, keepdim=True).values
    lse = torch.logsumexp(S, dim=-1, keepdim=True)
    P = torch.exp(S - lse)
    V = v.double()
    Amax = A.max(dim=-1, keepdim=True).values + (babs.max() if bias is not None else 0.0)
    eps = (C * dh * U * A  # f32 accumulation of the score over head_dim products (MFMA or VALU)
           + U * A  # the product acc * scale
           + U * (A + babs)  # the addition of the bias
           + U * (A + Amax)  # the subtraction of the row maximum
           + 2 * U * (A + Amax)  # __expf(x) = v_exp_f32(fl(x fl(log2 e))): two roundings of the argument, |x| <= |s| + |m|
           + 2 * U)  # v_exp_f32 (or expf): 1 ulp
    eps = torch.expm1(eps)
    if keep is not None:
        eps = torch.where(keep, eps, torch.zeros_like(eps))
    ebar = (P * eps).sum(-1, keepdim=True)
    # probs = e / l: the exponent error of e, that of l, the f32 sum of l over L terms, 1 / l (1 ulp), the product
    e_p = P * (eps + ebar / (1 - ebar) + (L + 3) * U) + TINY
    ref = P @ V
    err = e_p @ V.abs()  # the error of probs through the product
    err = err + rnd_bf16(P + e_p, bf16_p) @ V.abs()  # MFMA forms: probs rounded to bf16 for the PV product (VALU forms: f32)
    err = err + C * L * U * (P @ V.abs())  # f32 accumulation over L keys
    return P, e_p, ref, eb.store_bf16(ref, err)


def probs_fwd(q, k, v, scale: float, bias=None, bf16_p: bool = True):
    """(probs, probs_bound, out, out_bound) of attn_small_* / attn_cross_*: probs f32 [G, Nq, L], out bf16 [G, Nq, dh]"""
    G, Nq, L = q.shape[0], q.shape[1], k.shape[1]
    return _sliced(lambda a, b, c, d: _probs_fwd_slice(a, b, c, d, scale, bf16_p), G, Nq, L, q, k, v, bias)


def _probs_bwd_slice(q, k, v, do, probs, scale, bf16_p):
    dh, Nq, L = q.shape[2], q.shape[1], k.shape[1]
    Q, K, V, DO, P = q.double(), k.double(), v.double(), do.double(), probs.double()
    dP = DO @ V.transpose(-1, -2)
    e_dp = C * dh * U * (DO.abs() @ V.abs().transpose(-1, -2))  # f32 accumulation of dP over head_dim products
    dot = (P * dP).sum(-1, keepdim=True)
    e_dot = (P * e_dp).sum(-1, keepdim=True) + C * L * U * (P * dP.abs()).sum(-1, keepdim=True)  # f32 sum of P dP over L keys
    diff = dP - dot
    e_diff = e_dp + e_dot + U * (diff.abs() + e_dp + e_dot)  # one rounding of the difference
    dS = P * diff * scale
    e_ds = scale * P * e_diff + 2 * U * (dS.abs() + scale * P * e_diff)  # the products p * diff and * scale
    e_ds_r = e_ds + rnd_bf16(dS.abs() + e_ds, bf16_p)  # MFMA forms: dS rounded to bf16
    DOa, Ka, Qa = DO.abs(), K.abs(), Q.abs()
    dv = P.transpose(-1, -2) @ DO
    e_dv = rnd_bf16(P, bf16_p).transpose(-1, -2) @ DOa  # MFMA forms: probs rounded to bf16
    e_dv = e_dv + C * Nq * U * (P.transpose(-1, -2) @ DOa)  # f32 accumulation over Nq queries
    dq = dS @ K
    e_dq = e_ds_r @ Ka + C * L * U * (dS.abs() @ Ka)  # dS error; f32 accumulation over L keys
    dk = dS.transpose(-1, -2) @ Q
    e_dk = e_ds_r.transpose(-1, -2) @ Qa + C * Nq * U * (dS.abs().transpose(-1, -2) @ Qa)  # f32 accumulation over Nq queries
    return dS, eb.store_f32(dS, e_ds), dq, eb.store_bf16(dq, e_dq), dk, eb.store_bf16(dk, e_dk), dv, eb.store_bf16(dv, e_dv)


def probs_bwd(q, k, v, do, probs, scale: float, bf16_p: bool = True):
    """(ds, ds_bound, dq, dq_bound, dk, dk_bound, dv, dv_bound) from the backward's inputs, the forward's saved f32 probs included;
    ds f32 [G, Nq, L] is the cross kernels' scratch output (scale applied)"""
    G, Nq, L = q.shape[0], q.shape[1], k.shape[1]
    return _sliced(lambda *a: _probs_bwd_slice(*a, scale, bf16_p), G, Nq, L, q, k, v, do, probs)


# ------------------------------------------------------------------------------------------------------------------ fused QK-norm + RoPE
def qk_norm_rope(x, ssq, sc, cos, sin, N: int, H: int, rot: int, eps: float):
    """fp64 QK-RMSNorm + RoPE of the raw rows x [B * N, D] (the q or k third of qkv) with the statistics `ssq` [B * N] handed to the
    kernel as its input: (y [B * N, D], y_bound for the bf16 q_out / k_out, r [B * N], r_bound for the f32 rrms)"""
    M, D = x.shape
    X, s = x.double(), sc.double()
    inv_d = float(torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(D), dtype=torch.float32))
    r = torch.rsqrt(ssq.double() * inv_d + eps)
    # r = rsqrtf(ssq * inv_d + eps): the product and the sum (2 roundings of the argument: 1 U in r), v_rsq_f32 1 ulp (2 U), and the
    # argument's own value where inv_d = fl(1 / D) is taken as given; rounded up to 4 U as in test_wide_rows_gpu.py
    e_r = 4 * U * r
    y = X * r[:, None] * s
    e_y = (4 * U + 2 * U) * y.abs()  # r's error, the products x * r and * scale
    if rot:
        dh = D // H
        half = rot // 2
        yv = y.reshape(M // N, N, H, dh)
        ev = e_y.reshape(M // N, N, H, dh)
        c, n = cos.double()[None, :, None, :], sin.double()[None, :, None, :]
        a, b = yv[..., 0:rot:2], yv[..., 1:rot:2]
        ea, ebb = ev[..., 0:rot:2], ev[..., 1:rot:2]
        ra, rb = a * c - b * n, a * n + b * c
        mag = a.abs() * c.abs() + b.abs() * n.abs()
        magb = a.abs() * n.abs() + b.abs() * c.abs()
        # the inputs' errors through the rotation, the two products and the sum (fma or not: <= 2 roundings of the magnitudes)
        era = ea * c.abs() + ebb * n.abs() + 2 * U * mag
        erb = ea * n.abs() + ebb * c.abs() + 2 * U * magb
        yo, eo = yv.clone(), ev.clone()
        yo[..., 0:rot:2], yo[..., 1:rot:2] = ra, rb
        eo[..., 0:rot:2], eo[..., 1:rot:2] = era, erb
        assert half == cos.shape[1]
        y, e_y = yo.reshape(M, D), eo.reshape(M, D)
    return y, eb.store_bf16(y, e_y), r, e_r + eb.half_ulp(r, 24)


# ------------------------------------------------------------------------------------------------------------------ the check
def check(got, ref, bound, what: str, H: int = 1, rows: str = "query") -> float:
    """every element of got [G, N, d] (or [G, N]) within `bound` of `ref` (NaN fails); returns max |diff| / bound.  The failure message
    names the (batch, head), the row, its 32-row block (a wave's rows in the DiT kernels) and its 64-row block (as a key: the key
    block of the forward / phase A sweep) and, for a [G, Nq, Nk] matrix, the 64-key block of the column"""
    assert got.shape == ref.shape == bound.shape, (what, got.shape, ref.shape, bound.shape)
    g = got.to(ref.device).double()
    d = (g - ref).abs()
    ratio = d / bound.clamp_min(1e-300)
    ratio = torch.where(d == 0, torch.zeros_like(ratio), ratio)
    worst = float(torch.nan_to_num(ratio, nan=float("inf")).max()) if ratio.numel() else 0.0
    bad = ~(d <= bound)
    nbad = int(bad.sum())
    if nbad == 0:
        return worst
    flat = torch.nan_to_num(ratio, nan=float("inf")).reshape(-1)
    idx = int(flat.argmax())
    pos = []
    for n in reversed(got.shape):
        pos.append(idx % n)
        idx //= n
    pos = pos[::-1]
    gi, row = pos[0], pos[1]
    col = pos[2] if len(pos) > 2 else None
    gv, rv, bv = float(g[tuple(pos)]), float(ref[tuple(pos)]), float(bound[tuple(pos)])
    where = f"(batch {gi // H}, head {gi % H}), {rows} row {row}: 32-row block {row // 32}, 64-row block {row // 64}"
    if col is not None:
        where += f", column {col} (64-wide block {col // 64})"
    raise AssertionError(f"{what}: {nbad} of {got.numel()} elements outside their bound; worst at {where}: got {gv!r}, ref {rv!r}, "
                         f"|diff| {abs(gv - rv):.3e} > bound {bv:.3e}")
