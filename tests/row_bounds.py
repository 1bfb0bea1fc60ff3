"""fp64 references, element-wise bounds and runners of the row kernels of csrc/norm.hip, shared by tests/test_wide_rows_gpu.py
(1024 < D <= 4096, the *_rows_k forms) and tests/test_row_paths_gpu.py (D <= 1024, one wave per row); imported by the test modules,
not a conftest.  LayerNorm-modulate forward / backward (with and without the fused gated residual and the affine LayerNorm), the
per-token backward of the DDT decoder, the gated-residual backward and QK-RMSNorm + RoPE + head split forward / backward (row windows,
position tables, and the token-major in-place backward).  Bounds follow the arithmetic, in the style of tests/elementwise_bounds.py:
a row statistic over D terms in f32 carries c * D * 2^-24 of the magnitudes it sums, a column sum over R rows c * R * 2^-24 (the
previous value of a += output is one more term), local f32 steps a few 2^-24 of their terms, and a bf16 store half an ulp.  Outputs
sit in NaN-poisoned buffers whose guard regions are checked bit for bit after the call."""

from __future__ import annotations

import math

import torch

import elementwise_bounds as eb

DEV = "cuda"
U = 2.0**-24
C = 2.0
G = 4096  # guard elements on each side of a dense output


def rnd(seed, *shape, scale=1.0, dtype=torch.bfloat16):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(*shape, generator=g, device=DEV, dtype=torch.float32) * scale).to(dtype)


class Dense:
    """a dense tensor between two runs of G poisoned elements (init None: the tensor starts poisoned too)"""

    def __init__(self, shape, dtype, init=None):
        n = math.prod(shape)
        self.buf = eb.poison_(torch.empty(n + 2 * G, dtype=dtype, device=DEV))
        self.t = self.buf[G:G + n].view(*shape)
        if init is not None:
            self.t.copy_(init)

    def check(self, what, finite=True):
        assert bool(eb.is_poison(self.buf[:G]).all()) and bool(eb.is_poison(self.buf[-G:]).all()), f"{what}: guard written"
        if finite:
            assert bool(torch.isfinite(self.t.float()).all()), f"{what}: unwritten or non-finite elements"


def strided(values, pad=8):
    """values [R, D] as a view with row stride D + pad into a poisoned buffer (reads past a row see NaN)"""
    return eb.operand(values, values.shape[1] + pad)


def guarded_cols(rows, D, init):
    return eb.Guarded(rows, D, torch.float32, DEV, init=init)


def close(out, ref, err, what, bf16=True):
    eb.assert_within(out, ref, eb.store_bf16(ref, err) if bf16 else eb.store_f32(ref, err), tile=(1, out.shape[-1]), what=what)


def per_row(v, rows_per_mod):
    return v.double().repeat_interleave(rows_per_mod, 0)


# ------------------------------------------------------------------------------------------------ LayerNorm + modulate forward
def ln_fwd_ref(x, w, b, sc, sh, rpm, eps):
    D = x.shape[1]
    x = x.double()
    w = torch.ones(D, dtype=torch.float64, device=DEV) if w is None else w.double()
    b = torch.zeros(D, dtype=torch.float64, device=DEV) if b is None else b.double()
    s1, s2 = per_row(sc, rpm) + 1.0, per_row(sh, rpm)
    mu = x.mean(1, keepdim=True)
    rs = 1.0 / torch.sqrt(((x - mu) ** 2).mean(1, keepdim=True) + eps)
    xh = (x - mu) * rs
    out = (xh * w + b) * s1 + s2
    ax = x.abs().mean(1, keepdim=True)
    e_xh = C * D * U * (ax * rs + xh.abs())
    err = (w * s1).abs() * e_xh + 4 * U * ((xh * w * s1).abs() + (b * s1).abs() + s2.abs())
    return out, mu[:, 0], rs[:, 0], err, ax[:, 0]


def run_ln_fwd(ops, D, B, N, affine, gated, seed=0, check=True):
    M = B * N
    eps = 1e-6
    x = rnd(seed, M, D, scale=2.0) + 0.5
    w = (rnd(seed + 1, D, dtype=torch.float32) * 0.3 + 1.0) if affine else None
    b = (rnd(seed + 2, D, dtype=torch.float32) * 0.2) if affine else None
    sc, sh = strided(rnd(seed + 3, B, D, scale=0.3)), strided(rnd(seed + 4, B, D, scale=0.3))
    out, mean, rstd = Dense((M, D), torch.bfloat16), Dense((M,), torch.float32), Dense((M,), torch.float32)
    t = gate = xo = None
    if gated:
        t, gate = rnd(seed + 5, M, D), strided(rnd(seed + 6, B, D, scale=0.5))
        xo = Dense((M, D), torch.bfloat16)
    ops.ln_modulate_fwd(x, w, b, sc, sh, N, eps, out.t, mean.t, rstd.t, t=t, gate=gate, x_out=xo.t if gated else None)
    torch.cuda.synchronize()
    res = dict(out=out.t, mean=mean.t, rstd=rstd.t, x_out=xo.t if gated else None)
    if not check:
        return res
    for o, n in ((out, "out"), (mean, "mean"), (rstd, "rstd")) + (((xo, "x_out"),) if gated else ()):
        o.check(f"ln fwd D={D} {n}")
    xin = x
    if gated:  # x' = bf16(x + gate * t): one f32 rounding of the terms, then the bf16 store
        xr = x.double() + per_row(gate, N) * t.double()
        close(xo.t, xr, 2 * U * (x.double().abs() + (per_row(gate, N) * t.double()).abs()), f"ln fwd D={D} x_out")
        xin = xo.t  # the statistics are of what was stored
    ref, mu, rs, err, ax = ln_fwd_ref(xin, w, b, sc, sh, N, eps)
    close(out.t, ref, err, f"ln fwd D={D} affine={affine} gated={gated} out")
    close(mean.t[:, None], mu[:, None], (C * D * U * ax)[:, None], f"ln fwd D={D} mean", bf16=False)
    close(rstd.t[:, None], rs[:, None], (rs * (C * D * U + 4 * U))[:, None], f"ln fwd D={D} rstd", bf16=False)
    return res



# ------------------------------------------------------------------------------------------------ LayerNorm + modulate backward
def ln_bwd_parts(d, x, w, b, s1, mean, rstd):
    """per-row fp64 pieces shared by the per-sample and per-token backward; s1 = 1 + scale per row [M, D]"""
    D = x.shape[1]
    x, d = x.double(), d.double()
    w = torch.ones(D, dtype=torch.float64, device=DEV) if w is None else w.double()
    b = torch.zeros(D, dtype=torch.float64, device=DEV) if b is None else b.double()
    mu, rs = mean.double()[:, None], rstd.double()[:, None]
    xh = (x - mu) * rs
    e_xh = 2 * U * (x.abs() + mu.abs()) * rs
    dxh = d * s1 * w
    c1, c2 = dxh.mean(1, keepdim=True), (dxh * xh).mean(1, keepdim=True)
    dx = rs * (dxh - c1 - xh * c2)
    err = rs * (C * D * U * (dxh.abs().mean(1, keepdim=True) + xh.abs() * (dxh * xh).abs().mean(1, keepdim=True))
                + 8 * U * (dxh.abs() + c1.abs() + (xh * c2).abs()) + c2.abs() * e_xh + (dxh.abs() * e_xh).mean(1, keepdim=True))
    return dict(x=x, d=d, w=w, b=b, xh=xh, e_xh=e_xh, dx=dx, err=err)


def stats(x):
    x = x.double()
    mu = x.mean(1)
    rs = 1.0 / torch.sqrt(((x - mu[:, None]) ** 2).mean(1) + 1e-6)
    return mu.float(), rs.float()


def colsum(v, rpm):
    return v.view(-1, rpm, v.shape[1]).sum(1)


def run_ln_bwd(ops, D, B, N, affine, fused, dres_on, seed=0, check=True, init=False):
    """init: dscale / dshift / dgate / dwb start from non-zero values (they are +=): one more addend of each f32 column sum"""
    M = B * N
    x = rnd(seed, M, D, scale=2.0) + 0.25
    d = rnd(seed + 1, M, D)
    w = (rnd(seed + 2, D, dtype=torch.float32) * 0.3 + 1.0) if affine else None
    b = (rnd(seed + 3, D, dtype=torch.float32) * 0.2) if affine else None
    sc = strided(rnd(seed + 4, B, D, scale=0.3))
    mean, rstd = stats(x)
    dres = rnd(seed + 5, M, D) if dres_on else None
    dx = Dense((M, D), torch.bfloat16)
    def start(k, *shape):
        return rnd(seed + k, *shape, scale=0.5, dtype=torch.float32) if init else torch.zeros(*shape, device=DEV)

    i_sc, i_sh, i_g, i_wb = start(8, B, D), start(9, B, D), start(10, B, D), start(11, B, 2, D)
    dsc, dsh = guarded_cols(B, D, i_sc), guarded_cols(B, D, i_sh)
    dg = guarded_cols(B, D, i_g) if fused else None
    dwb = Dense((B, 2, D), torch.float32, init=i_wb) if affine else None
    gt = gg = dt = None
    if fused:
        gt, gg, dt = rnd(seed + 6, M, D), strided(rnd(seed + 7, B, D, scale=0.5)), Dense((M, D), torch.bfloat16)
    # ops.ln_modulate_bwd passes dscale's row stride for dgate: give all three the same layout
    ops.ln_modulate_bwd(d, x, w, b, sc, N, mean, rstd, dres, dx.t, dsc.win, dsh.win, dwb.t if affine else None, gate_t=gt, gate=gg,
                        dt=dt.t if fused else None, dgate=dg.win if fused else None)
    torch.cuda.synchronize()
    res = dict(dx=dx.t, dt=dt.t if fused else None)
    if not check:
        return res
    dx.check(f"ln bwd D={D} dx")
    dsc.check("dscale")
    dsh.check("dshift")
    s1 = per_row(sc, N) + 1.0
    P = ln_bwd_parts(d, x, w, b, s1, mean, rstd)
    ref, err = P["dx"], P["err"]
    if dres_on:
        ref, err = ref + dres.double(), err + 2 * U * (ref.abs() + dres.double().abs())
    what = f"ln bwd D={D} rows={B}x{N} affine={affine} fused={fused} dres={dres_on}"
    close(dx.t, ref, err, what + " dx")
    dd, xh = P["d"], P["xh"]
    S1, S2 = colsum(dd, N), colsum(dd * xh, N)
    e1 = (C * N + 4) * U * colsum(dd.abs(), N)
    e2 = (C * N + 4) * U * colsum((dd * xh).abs(), N) + colsum(dd.abs() * P["e_xh"], N)
    wv, bv = P["w"], P["b"]

    def e0(i):  # the initial value among the addends of the column sum
        return (C * N + 4) * U * i.double().abs()

    close(dsc.win, i_sc.double() + wv * S2 + bv * S1,
          wv.abs() * e2 + bv.abs() * e1 + 2 * U * ((wv * S2).abs() + (bv * S1).abs()) + e0(i_sc), what + " dscale", bf16=False)
    close(dsh.win, i_sh.double() + S1, e1 + e0(i_sh), what + " dshift", bf16=False)
    if affine:
        dwb.check("dwb")
        sp = sc.double() + 1.0
        close(dwb.t[:, 0], i_wb[:, 0].double() + sp * S2, sp.abs() * e2 + 2 * U * (sp * S2).abs() + e0(i_wb[:, 0]), what + " dw", bf16=False)
        close(dwb.t[:, 1], i_wb[:, 1].double() + sp * S1, sp.abs() * e1 + 2 * U * (sp * S1).abs() + e0(i_wb[:, 1]), what + " db", bf16=False)
    if fused:  # dt = gate * dx and dgate = sum dx * t, of dx as stored
        dt.check("dt")
        dg.check("dgate")
        dxs = dx.t.double()
        gr = per_row(gg, N)
        close(dt.t, dxs * gr, 2 * U * (dxs * gr).abs(), what + " dt")
        p = dxs * gt.double()
        close(dg.win, i_g.double() + colsum(p, N), (C * N + 4) * U * colsum(p.abs(), N) + e0(i_g), what + " dgate", bf16=False)
    return res



# ------------------------------------------------------------------------------------------------ per-token backward (DDT decoder)
def run_ln_bwd_tok(ops, D, M, affine, fused, seed=0, n_part=3, check=True):
    x = rnd(seed, M, D, scale=2.0) - 0.25
    d = rnd(seed + 1, M, D)
    w = (rnd(seed + 2, D, dtype=torch.float32) * 0.3 + 1.0) if affine else None
    b = (rnd(seed + 3, D, dtype=torch.float32) * 0.2) if affine else None
    sc = strided(rnd(seed + 4, M, D, scale=0.3))
    mean, rstd = stats(x)
    dres = rnd(seed + 5, M, D)
    dx = Dense((M, D), torch.bfloat16)
    # dscale / dshift / dgate: bf16 row windows with one shared row stride (the modulation-gradient matrix)
    dmod = eb.Guarded(M, 3 * D, torch.bfloat16, DEV)
    dsc, dsh, dg = dmod.win[:, :D], dmod.win[:, D:2 * D], dmod.win[:, 2 * D:]
    dwb = Dense((n_part, 2, D), torch.float32, init=torch.zeros(n_part, 2, D, device=DEV)) if affine else None
    gt = gg = dt = None
    if fused:
        gt, gg, dt = rnd(seed + 6, M, D), strided(rnd(seed + 7, M, D, scale=0.5)), Dense((M, D), torch.bfloat16)
    ops.ln_modulate_bwd_tok(d, x, w, b, sc, mean, rstd, dres, dx.t, dsc, dsh, dwb.t if affine else None, gate_t=gt, gate=gg,
                            dt=dt.t if fused else None, dgate=dg if fused else None)
    torch.cuda.synchronize()
    res = dict(dx=dx.t, dscale=dsc, dshift=dsh, dgate=dg if fused else None, dt=dt.t if fused else None)
    if not check:
        return res
    what = f"ln bwd tok D={D} M={M} affine={affine} fused={fused}"
    dx.check(what + " dx")
    hit = dmod.mask & ~eb.is_poison(dmod.buf)
    assert not bool(hit.any()), what + ": guard of the modulation-gradient matrix written"
    s1 = sc.double() + 1.0
    P = ln_bwd_parts(d, x, w, b, s1, mean, rstd)
    ref, err = P["dx"] + dres.double(), P["err"] + 2 * U * (P["dx"].abs() + dres.double().abs())
    close(dx.t, ref, err, what + " dx")
    dd, xh, wv, bv = P["d"], P["xh"], P["w"], P["b"]
    r = dd * (xh * wv + bv)
    close(dsc, r, 4 * U * dd.abs() * ((xh * wv).abs() + bv.abs()) + (dd * wv).abs() * P["e_xh"], what + " dscale")
    assert torch.equal(dsh.view(torch.int16), d.view(torch.int16)), what + ": dshift is dout bit for bit"
    if fused:
        dt.check("dt")
        dxs = dx.t.double()
        close(dg, dxs * gt.double(), 2 * U * (dxs * gt.double()).abs(), what + " dgate")
        close(dt.t, dxs * gg.double(), 2 * U * (dxs * gg.double()).abs(), what + " dt")
    else:
        assert bool(eb.is_poison(dg).all()), what + ": dgate written without the fused gate"
    if affine:
        dwb.check("dwb")
        dy = dd * s1
        tot = dwb.t.sum(0).double()  # the n_part slabs hold a split of the column sums
        e_dw = (C * M + 4) * U * (dy * xh).abs().sum(0) + (dy.abs() * P["e_xh"]).sum(0)
        close(tot[0][None], (dy * xh).sum(0)[None], e_dw[None], what + " dw", bf16=False)
        close(tot[1][None], dy.sum(0)[None], ((C * M + 4) * U * dy.abs().sum(0))[None], what + " db", bf16=False)
    return res



# ------------------------------------------------------------------------------------------------ gated residual backward
def run_gate_bwd(ops, D, B, N, seed=0, check=True):
    M = B * N
    d, t = rnd(seed, M, D), rnd(seed + 1, M, D)
    gate = strided(rnd(seed + 2, B, D, scale=0.5))
    dt = Dense((M, D), torch.bfloat16)
    dg = guarded_cols(B, D, None)  # plain stores: the window starts poisoned and must be overwritten
    ops.gate_bwd(d, t, gate, N, dt.t, dg.win)
    torch.cuda.synchronize()
    res = dict(dt=dt.t, dgate=dg.win)
    if not check:
        return res
    what = f"gate bwd D={D} rows={B}x{N}"
    dt.check(what + " dt")
    dg.check(what + " dgate")
    gr = per_row(gate, N)
    close(dt.t, d.double() * gr, 2 * U * (d.double() * gr).abs(), what + " dt")
    p = d.double() * t.double()
    close(dg.win, colsum(p, N), (C * N + 4) * U * colsum(p.abs(), N), what + " dgate", bf16=False)
    return res



# ------------------------------------------------------------------------------------------------ QK RMSNorm + RoPE + head split
def rope_tables(T, rot, seed):
    ang = torch.rand(T, rot // 2, generator=torch.Generator(device=DEV).manual_seed(seed), device=DEV, dtype=torch.float64) * 6.3
    return ang.cos().float().contiguous(), ang.sin().float().contiguous()


def rotate(a, cs, sn, rot, inverse=False):
    """pairs (2i, 2i + 1) of the first rot columns of every head, a [M, H, dh] fp64; cs / sn [M, rot / 2] per row"""
    out, err = a.clone(), torch.zeros_like(a)
    c, s = cs.double()[:, None, :], sn.double()[:, None, :]
    x0, x1 = a[..., 0:rot:2], a[..., 1:rot:2]
    if inverse:
        out[..., 0:rot:2], out[..., 1:rot:2] = x0 * c + x1 * s, -x0 * s + x1 * c
    else:
        out[..., 0:rot:2], out[..., 1:rot:2] = x0 * c - x1 * s, x0 * s + x1 * c
    t = (x0 * c).abs() + (x1 * s).abs() + (x0 * s).abs() + (x1 * c).abs()
    err[..., 0:rot:2], err[..., 1:rot:2] = 2 * U * t, 2 * U * t
    return out, err


def heads(t, B, N, H, dh, n_off, n_dst):
    """[B, H, n_dst, dh] -> the window rows as [B * N, H, dh]"""
    return t[:, :, n_off:n_off + N].permute(0, 2, 1, 3).reshape(B * N, H, dh)


def qk_bwd_ref(qkv, scales, cr, sr, rrms, grads, H, dh, rot):
    """for q and k: (d x ref, its bound, dscale column sums, their bound) from the gradients after norm + RoPE, grads[i] [M, H, dh]
    (bf16 values), the pre-norm qkv rows, the per-row table entries cr / sr and the device's rrms [M, 2]"""
    M, D = qkv.shape[0], H * dh
    x = qkv.double().view(M, 3, H, dh)
    out = []
    for i, w in enumerate(scales):
        xi = x[:, i]
        r = rrms[:, i].double()[:, None, None]
        g, e_g = rotate(grads[i].double(), cr, sr, rot, inverse=True)
        gw = g * w.double().view(H, dh)
        m = (gw * xi).reshape(M, D).mean(1)[:, None, None] * r ** 3
        ref = r * gw - xi * m
        err = (r * w.double().view(H, dh).abs() * e_g + C * D * U * xi.abs() * r ** 3 * (gw * xi).abs().reshape(M, D).mean(1)[:, None, None]
               + 4 * U * ((r * gw).abs() + (xi * m).abs()))
        p = (g * xi * r).reshape(M, D)
        e_p = (C * M + 4) * U * p.abs().sum(0) + (e_g * xi.abs() * r).reshape(M, D).sum(0)
        out.append((ref.reshape(M, D), err.reshape(M, D), p.sum(0), e_p))
    return out


def run_qk(ops, B, N, H, dh, rot, window, seed=0, check=True, v_on=True):
    D, M = H * dh, B * N
    qkv = rnd(seed, M, 3 * D, scale=1.5)
    sq, sk = rnd(seed + 1, D, dtype=torch.float32) * 0.3 + 1.0, rnd(seed + 2, D, dtype=torch.float32) * 0.3 + 1.0
    if window:
        n_off, n_dst, T = 7, N + 19, N + 40
        pos = torch.randint(0, T, (M,), generator=torch.Generator(device=DEV).manual_seed(seed + 3), device=DEV, dtype=torch.int32)
    else:
        n_off, n_dst, T, pos = 0, N, N, None
    cs, sn = rope_tables(T, rot, seed + 4)
    q, k, v = (Dense((B, H, n_dst, dh), torch.bfloat16) for _ in range(3))
    rr = Dense((M, 2), torch.float32)
    ops.qk_norm_rope_fwd(qkv, sq, sk, cs, sn, q.t, k.t, v.t if v_on else None, rr.t, B, N, H, dh, rot, eps=1e-6, pos=pos, n_off=n_off)
    dq, dk, dv = rnd(seed + 5, B, H, n_dst, dh), rnd(seed + 6, B, H, n_dst, dh), rnd(seed + 7, B, H, n_dst, dh)
    dqkv = Dense((M, 3 * D), torch.bfloat16)
    dsc = Dense((2, D), torch.float32, init=torch.zeros(2, D, device=DEV))
    ops.qk_norm_rope_bwd(dq, dk, dv if v_on else None, qkv, sq, sk, cs, sn, rr.t, dqkv.t, dsc.t, B, N, H, dh, rot, pos=pos, n_off=n_off)
    torch.cuda.synchronize()
    res = dict(q=q.t, k=k.t, v=v.t, rrms=rr.t, dqkv=dqkv.t, dscale=dsc.t)
    if not check:
        return res
    what = f"qk D={D} rows={B}x{N} rot={rot} window={window}"
    rows = (pos.long() if pos is not None else torch.arange(M, device=DEV) % N)
    cr, sr = cs[rows], sn[rows]
    # the rows outside the window [n_off, n_off + N) of every (sample, head) stay poisoned
    for o, nm in ((q, "q"), (k, "k")) + (((v, "v"),) if v_on else ()):
        o.check(what + " " + nm, finite=False)
        inside = torch.zeros(n_dst, dtype=torch.bool, device=DEV)
        inside[n_off:n_off + N] = True
        assert bool(eb.is_poison(o.t[:, :, ~inside]).all()), f"{what}: {nm} written outside its row window"
        assert bool(torch.isfinite(o.t[:, :, inside].float()).all()), f"{what}: {nm} window not written"
    if not v_on:
        assert bool(eb.is_poison(v.t).all())
    rr.check(what + " rrms")
    dqkv.check(what + " dqkv", finite=v_on)
    dsc.check(what + " dscale")
    x = qkv.double().view(M, 3, H, dh)
    rs_ref = []
    for i, (o, w) in enumerate(((q, sq), (k, sk))):
        xi = x[:, i]
        ms = (xi ** 2).reshape(M, D).mean(1)
        r = 1.0 / torch.sqrt(ms + 1e-6)
        rs_ref.append(r)
        close(rr.t[:, i:i + 1], r[:, None], (r * (C * D * U + 4 * U))[:, None], what + " rrms", bf16=False)
        xn = xi * r[:, None, None] * w.double().view(H, dh)
        e_n = xn.abs() * (C * D * U + 4 * U)
        ref, e_r = rotate(xn, cr, sr, rot)
        e_rot = e_r.clone()
        e_rot[..., 0:rot:2] += e_n[..., 0:rot:2] + e_n[..., 1:rot:2]
        e_rot[..., 1:rot:2] += e_n[..., 0:rot:2] + e_n[..., 1:rot:2]
        e_rot[..., rot:] += e_n[..., rot:]
        close(heads(o.t, B, N, H, dh, n_off, n_dst).reshape(M, D), ref.reshape(M, D), e_rot.reshape(M, D), f"{what} {'qk'[i]}")
    if v_on:
        assert torch.equal(heads(v.t, B, N, H, dh, n_off, n_dst).reshape(M, D).view(torch.int16),
                           qkv[:, 2 * D:].contiguous().view(torch.int16)), what + ": v is the v third bit for bit"
    # backward: the device's rrms are the kernel's inputs
    grads = [heads(gsrc, B, N, H, dh, n_off, n_dst) for gsrc in (dq, dk)]
    for i, (ref, err, ps, e_p) in enumerate(qk_bwd_ref(qkv, (sq, sk), cr, sr, rr.t, grads, H, dh, rot)):
        close(dqkv.t[:, i * D:(i + 1) * D], ref, err, f"{what} d{'qk'[i]}")
        close(dsc.t[i:i + 1], ps[None], e_p[None], f"{what} dscale {'qk'[i]}", bf16=False)
    if v_on:
        assert torch.equal(dqkv.t[:, 2 * D:].contiguous().view(torch.int16),
                           heads(dv, B, N, H, dh, n_off, n_dst).reshape(M, D).contiguous().view(torch.int16)), what + ": dv bit for bit"
    return res



# ------------------------------------------------------------------------------------------------ token-major, in-place QK backward
PART_ROWS = 1024  # rows of [2, D] the scale-gradient scratch must hold (ops.qk_norm_rope_bwd_inplace)


def inplace_grid(M):
    """workgroups of dl_qk_norm_rope_bwd_inplace: each writes one [2, D] row of the scratch"""
    per = 64 if M >= 32768 else 16
    return min((M + per - 1) // per, 768)


def run_qk_inplace(ops, B, N, H, dh, rot, with_pos, seed=0, check=True):
    """dqkv [M, 3D] arrives with the gradients after norm + RoPE in its q / k thirds (token-major) and dv in its v third; the q / k
    thirds leave as the gradients of the pre-norm q / k, the v third bit for bit; dscale [2, D] += through a poisoned scratch"""
    D, M = H * dh, B * N
    qkv = rnd(seed, M, 3 * D, scale=1.5)
    sq, sk = rnd(seed + 1, D, dtype=torch.float32) * 0.3 + 1.0, rnd(seed + 2, D, dtype=torch.float32) * 0.3 + 1.0
    T = N + 40 if with_pos else N
    pos = (torch.randint(0, T, (M,), generator=torch.Generator(device=DEV).manual_seed(seed + 3), device=DEV, dtype=torch.int32)
           if with_pos else None)
    cs, sn = rope_tables(T, rot, seed + 4)
    q, k, v = (torch.empty(B, H, N, dh, device=DEV, dtype=torch.bfloat16) for _ in range(3))
    rr = torch.empty(M, 2, device=DEV)
    ops.qk_norm_rope_fwd(qkv, sq, sk, cs, sn, q, k, v, rr, B, N, H, dh, rot, eps=1e-6, pos=pos)
    g_in = rnd(seed + 5, M, 3 * D)
    dqkv = Dense((M, 3 * D), torch.bfloat16, init=g_in)
    i_sc = rnd(seed + 6, 2, D, dtype=torch.float32) * 0.5
    dsc = Dense((2, D), torch.float32, init=i_sc)
    part = Dense((PART_ROWS * 2 * D,), torch.float32)  # poisoned on entry
    ok = ops.qk_norm_rope_bwd_inplace(qkv, sq, sk, cs, sn, rr, dqkv.t, dsc.t, part.t, B, N, H, dh, rot, pos=pos)
    torch.cuda.synchronize()
    res = dict(ok=ok, dqkv=dqkv.t, dscale=dsc.t, g_in=g_in, i_sc=i_sc)
    if not check or not ok:
        return res
    what = f"qk in place D={D} ({H} x {dh}) rows={B}x{N} rot={rot} pos={with_pos}"
    dqkv.check(what + " dqkv")
    dsc.check(what + " dscale")
    part.check(what + " scratch", finite=False)
    used = inplace_grid(M) * 2 * D
    assert bool(torch.isfinite(part.t[:used]).all()), what + ": scratch rows of the launched workgroups not all written"
    assert bool(eb.is_poison(part.t[used:]).all()), what + ": scratch written beyond grid * 2 * D"
    rows = pos.long() if pos is not None else torch.arange(M, device=DEV) % N
    grads = [g_in[:, i * D:(i + 1) * D].reshape(M, H, dh) for i in range(2)]
    for i, (ref, err, ps, e_p) in enumerate(qk_bwd_ref(qkv, (sq, sk), cs[rows], sn[rows], rr, grads, H, dh, rot)):
        close(dqkv.t[:, i * D:(i + 1) * D], ref, err, f"{what} d{'qk'[i]}")
        i0 = i_sc[i].double()
        close(dsc.t[i:i + 1], (i0 + ps)[None], (e_p + (C * M + 4) * U * i0.abs())[None], f"{what} dscale {'qk'[i]}", bf16=False)
    assert torch.equal(dqkv.t[:, 2 * D:].contiguous().view(torch.int16), g_in[:, 2 * D:].contiguous().view(torch.int16)), what + ": v third changed"
    return res
