"""fp64 references and element-wise error bounds for the GroupNorm kernels of csrc/unet.hip (imported by the test modules; not a
conftest).  Builds on tests/elementwise_bounds.py: the same constants, store terms and poisoned buffers.

Layout: x, out, dout, dres, dx are [B, HW, C] bf16 (NHWC token rows), group g owns channels g * C/G .. (g + 1) * C/G - 1, the
statistics are f32 [B, G, 2] = (mean, rstd), w / b are f32 [C], the FiLM operands scale / shift bf16 [B, C].

    forward     out = act((xhat w + b) (1 + scale) + shift),  xhat = (x - mean) rstd,  rstd = (var + eps)^-1/2
    backward    dh = dout act'(h), dy = dh (1 + scale);  per (sample, channel): S0 = sum dh y, S1 = sum dh, S2 = sum dy xhat, S3 = sum dy
                dfilm_scale = bf16(S0), dfilm_shift = bf16(S1), dw += sum_b S2, db += sum_b S3
                per (sample, group): A = sum_c w S3 / n, Bv = sum_c w S2 / n, n = HW C/G;  dx = rstd (dy w - A - xhat Bv) + dres

Every bound is a sum of named terms, one per rounding the kernels perform.  Two rules keep them honest:
  * the statistics bound follows the summation DEPTH of the form under test (the longest chain of f32 additions one addend passes
    through: pixels per lane, lanes, channels per group -- stats_depth below), applied to mean|x| for the mean and to the CENTRED second
    moment for the variance.  It holds no mu^2 / var term: GroupNorm of exactly representable inputs is well conditioned, and a kernel
    that forms E[x^2] - mu^2 in f32 owes that amplification to its formula, not to the operation;
  * the backward takes the f32 statistics as given operands (that is the kernel's contract: it never recomputes them), and its sums
    are bounded order-free, gamma_terms * sum |term|, because pixel ranges, LDS atomics and global atomics fix no order.
"""

from __future__ import annotations

import torch

import elementwise_bounds as eb

U = eb.U32
ACC_C = eb.ACC_C
EPS = 1e-5
CLASSES = ("scaled", "offset4", "offset32", "const", "spike")


# ------------------------------------------------------------------------------------------------------------------ summation depth
def _cdiv(a, b):
    return -(-a // b)


def stats_depth(form: str, HW: int, C: int, G: int) -> int:
    """longest chain of f32 additions in the statistics of one form.
    stats:        256 / (C/8) pixel lanes walk the pixels; thread g then adds lanes x channels of its group in one serial chain
    stats_atomic: one thread per chunk walks every pixel; C/G LDS atomics per group
    fused16 / fused8 (NCH = 16 / 8, 256 / NCH pixel lanes): pixels per lane, log2(64 / NCH) shuffle levels, then 8 threads per group
                  add 4 wave partials x ceil(cg / 8) channels each and meet in 3 shuffles
    fused12:      21 pixel lanes, every lane leaves a partial: 21 partials x ceil(cg / 8) channels, 3 shuffles"""
    cg = C // G
    if form == "stats":
        npl = 256 // (C // 8)
        return _cdiv(HW, npl) + npl * cg
    if form == "stats_atomic":
        return HW + cg
    if form == "fused16":
        return _cdiv(HW, 16) + 2 + 4 * _cdiv(cg, 8) + 3
    if form == "fused8":
        return _cdiv(HW, 32) + 3 + 4 * _cdiv(cg, 8) + 3
    if form == "fused12":
        return _cdiv(HW, 21) + 21 * _cdiv(cg, 8) + 3
    raise ValueError(form)


# ------------------------------------------------------------------------------------------------------------------ inputs
def make_x(cls: str, B: int, HW: int, C: int, G: int, gen: torch.Generator, device) -> torch.Tensor:
    """bf16 [B, HW, C] of one input class (CLASSES).
    scaled:   per-channel scale in [0.5, 2.5] and offset 1.5 N(0, 1): neighbouring groups differ, a mis-booked chunk shows
    offset4 / offset32: group mean at 4 x / 32 x the group std (signs alternate between groups); the realised ratio after the bf16
              rounding is asserted where a group has >= 64 elements
    const:    as scaled, with every element of two groups equal (true variance 0)
    spike:    as scaled / 4, one pixel 2^6 times the rest"""
    cg = C // G
    n = lambda *s: torch.randn(s, generator=gen, device=device)  # noqa: E731
    u = lambda *s: torch.rand(s, generator=gen, device=device)  # noqa: E731
    if cls in ("offset4", "offset32"):
        ratio = 4.0 if cls == "offset4" else 32.0
        sd = (0.5 + 1.5 * u(1, 1, G)).repeat_interleave(cg, 2)
        sign = (1.0 - 2.0 * (torch.arange(G, device=device) % 2)).repeat_interleave(cg)[None, None, :]
        x = (n(B, HW, C) * sd + ratio * sd * sign).to(torch.bfloat16)
        if HW * cg >= 64:
            xg = x.double().reshape(B, HW, G, cg)
            real = xg.mean((1, 3)).abs() / xg.var((1, 3), unbiased=False).sqrt()
            assert float(real.min()) > 0.7 * ratio and float(real.max()) < 1.4 * ratio, (cls, float(real.min()), float(real.max()))
        return x
    x = n(B, HW, C) * (0.5 + 2.0 * u(1, 1, C)) + 1.5 * n(1, 1, C)
    if cls == "const":
        xg = x.reshape(B, HW, G, cg)
        xg[0, :, 1 % G, :] = 2.71875  # (exact in bf16)
        xg[B - 1, :, G - 1, :] = -0.3984375
    elif cls == "spike":
        x = x * 0.25
        x[:, HW // 2, :] *= 64.0
    else:
        assert cls == "scaled", cls
    return x.to(torch.bfloat16)


# ------------------------------------------------------------------------------------------------------------------ forward
def _per_channel(t, cg):
    """[B, G] -> [B, 1, C]"""
    return t.repeat_interleave(cg, 1)[:, None, :]


def fwd_ref(x, w, b, scale, shift, silu: bool, G: int, eps: float, depth: int):
    """-> {"mean": (ref, bound), "rstd": (ref, bound), "out": (ref, bound)}: mean / rstd fp64 [B, G], out fp64 [B, HW, C]"""
    B, HW, C = x.shape
    cg = C // G
    X = x.double()
    Xg = X.reshape(B, HW, G, cg)
    mu = Xg.mean((1, 3))
    var = (Xg - mu[:, None, :, None]).square().mean((1, 3))
    r = (var + eps).rsqrt()
    acc = ACC_C * depth * U
    # mean: the f32 sum of x over `depth` additions (of mean|x| per term), then the division by n
    e_mu = acc * Xg.abs().mean((1, 3)) + U * mu.abs()
    # variance: every (x - m)^2 carries the roundings of the difference (twice) and of the square, their sum `depth` additions, the
    # division one more; m is the f32 mean, off by e_mu, which moves the centred moment by e_mu^2 (the cross term vanishes)
    e_var = (acc + 4 * U) * var + e_mu.square()
    # rstd: var + eps rounded, rsqrt to 1 ulp; d rstd / d var = -rstd / (2 (var + eps))
    e_r = 0.5 * r / (var + eps) * e_var + 3 * U * r
    res = {"mean": (mu, eb.store_f32(mu, e_mu)), "rstd": (r, eb.store_f32(r, e_r))}
    # the apply pass reads the f32 statistics: their error plus half an ulp of the store
    muc, rc = _per_channel(mu, cg), _per_channel(r, cg)
    e_muc, e_rc = _per_channel(res["mean"][1], cg), _per_channel(res["rstd"][1], cg)
    W, Bb = w.double()[None, None, :], b.double()[None, None, :]
    d = X - muc
    xh = d * rc
    e_xh = rc * e_muc + d.abs() * e_rc + e_muc * e_rc + 2 * U * xh.abs()  # the difference and the product, one rounding each
    y = xh * W + Bb
    e = W.abs() * e_xh + 2 * U * ((xh * W).abs() + Bb.abs())  # product and sum
    if scale is not None:
        s1, s2 = 1.0 + scale.double()[:, None, :], shift.double()[:, None, :]
        h = y * s1 + s2
        e = s1.abs() * e + U * (s1 * y).abs() + 2 * U * ((y * s1).abs() + s2.abs())  # 1 + scale rounded; product and sum
    else:
        h = y
    if silu:
        h, e = eb.silu(h, e)
    res["out"] = (h, eb.store_bf16(h, e))
    return res


# ------------------------------------------------------------------------------------------------------------------ backward
def dsilu(h):
    s = torch.sigmoid(h)
    return s * (1.0 + h * (1.0 - s))


def bwd_ref(dout, x, stats, w, b, scale, shift, silu: bool, dres, dw0, db0, G: int):
    """the backward from the f32 statistics as given.  -> {"dx", "dw", "db"[, "dfilm_scale", "dfilm_shift"]: (ref, bound)}:
    dx fp64 [B, HW, C], dw / db [C] (from the initial values dw0 / db0: += semantics), dfilm_* [B, C]"""
    B, HW, C = x.shape
    cg = C // G
    n = HW * cg
    X, D = x.double(), dout.double()
    muc, rc = _per_channel(stats[..., 0].double(), cg), _per_channel(stats[..., 1].double(), cg)
    W, Bb = w.double()[None, None, :], b.double()[None, None, :]
    xh = (X - muc) * rc
    e_xh = 2 * U * xh.abs()  # the difference and the product
    y = xh * W + Bb
    e_y = W.abs() * e_xh + 2 * U * ((xh * W).abs() + Bb.abs())
    if scale is not None:
        s1, s2 = 1.0 + scale.double()[:, None, :], shift.double()[:, None, :]
        h = y * s1 + s2
        e_h = s1.abs() * e_y + U * (s1 * y).abs() + 2 * U * ((y * s1).abs() + s2.abs())
    else:
        s1, h, e_h = torch.ones_like(muc), y, e_y
    if silu:
        # act'(h) = s (1 + h (1 - s)) at the recomputed pre-activation: |act''| <= 1/2 times the error of h, the device sigmoid's
        # relative error rho (exp argument, v_exp, v_rcp, the add), which reaches 1 - s as an ABSOLUTE rho s, and three more roundings
        s = torch.sigmoid(h)
        da = s * (1.0 + h * (1.0 - s))
        rho = (1.5 * (h.abs() + e_h) + 5.0) * U
        e_da = 0.5 * e_h + (rho + 3 * U) * da.abs() + s * h.abs() * (rho * s + 2 * U)
    else:
        da, e_da = torch.ones_like(h), torch.zeros_like(h)
    dh = D * da
    e_dh = D.abs() * e_da + U * dh.abs()
    dy = dh * s1
    e_dy = s1.abs() * e_dh + 2 * U * dy.abs()
    # sums over the HW pixels, order-free; the fused form takes S0 as w P + b Q (P = sum dh xhat, Q = sum dh) and S2 / S3 as
    # (1 + scale) P / Q: the magnitudes below are those of the expanded terms, which cover both ways of grouping
    g_hw = (ACC_C * HW + 4) * U
    ymag = W.abs() * xh.abs() + Bb.abs()
    t0, t2 = e_dh * ymag + dh.abs() * e_y, e_dy * xh.abs() + dy.abs() * e_xh  # errors of the terms themselves
    S0, m0 = (dh * y).sum(1), (dh.abs() * ymag).sum(1)
    S1, m1 = dh.sum(1), dh.abs().sum(1)
    S2, m2 = (dy * xh).sum(1), (dy.abs() * xh.abs()).sum(1)
    S3, m3 = dy.sum(1), dy.abs().sum(1)
    res = {}
    if scale is not None:
        res["dfilm_scale"] = (S0, eb.store_bf16(S0, t0.sum(1) + g_hw * m0))
        res["dfilm_shift"] = (S1, eb.store_bf16(S1, e_dh.sum(1) + g_hw * m1))
    # dw / db: one f32 sum of the initial value and B HW terms, in whatever order the atomics land
    g_b = (ACC_C * (B * HW + 1) + 4) * U
    dw, db = dw0.double() + S2.sum(0), db0.double() + S3.sum(0)
    res["dw"] = (dw, eb.store_f32(dw, t2.sum((0, 1)) + g_b * (dw0.double().abs() + m2.sum(0))))
    res["db"] = (db, eb.store_f32(db, e_dy.sum((0, 1)) + g_b * (db0.double().abs() + m3.sum(0))))
    # group sums over HW C/G terms, the product with w and the division by n two roundings more
    g_n = (ACC_C * n + 4) * U
    Wc = w.double()[None, :]
    grp = lambda t: t.reshape(B, G, cg).sum(2)  # noqa: E731
    A, e_A = grp(Wc * S3) / n, (grp(Wc.abs() * e_dy.sum(1)) + g_n * grp(Wc.abs() * m3)) / n
    Bv, e_B = grp(Wc * S2) / n, (grp(Wc.abs() * t2.sum(1)) + g_n * grp(Wc.abs() * m2)) / n
    Ac, Bc, e_Ac, e_Bc = (_per_channel(t, cg) for t in (A, Bv, e_A, e_B))
    inner = dy * W - Ac - xh * Bc
    dx = rc * inner
    e = rc * (W.abs() * e_dy + e_Ac + xh.abs() * e_Bc + Bc.abs() * e_xh) + 4 * U * rc * ((dy * W).abs() + Ac.abs() + (xh * Bc).abs())
    if dres is not None:
        dx = dx + dres.double()
        e = e + U * (dx.abs() + e)
    res["dx"] = (dx, eb.store_bf16(dx, e))
    return res


def worst_ratio(out, ref, bound) -> float:
    """max |out - ref| / bound (NaN counts as inf)"""
    d = (out.to(ref.device).double() - ref).abs() / bound
    return float(torch.nan_to_num(d, nan=float("inf")).max())
