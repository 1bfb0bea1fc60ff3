"""What the bounds of tests/bf16_aux_bounds.py admit and what they reject, on the CPU.

For every kind of bound the kernel's arithmetic is emulated in torch -- f32 steps in the kernel's order, then the bf16 store -- and
must sit inside the bound (the worst ratio is printed); a set of mutants (a truncating store, a dropped row, a wrong divisor, ...)
must land outside it, with |diff| / bound > 1 on at least one element or a bit-compare that fails.  Every input generator must give
finite references and finite bounds.
"""

from __future__ import annotations

import math

import pytest
import torch

import bf16_aux_bounds as ab
import f32_bounds as fb

BF, F32 = torch.bfloat16, torch.float32
DEV = "cpu"


def gen(seed=0):
    return torch.Generator().manual_seed(seed)


def r16(g, *s, scale=1.0):
    return (scale * torch.randn(s, generator=g)).to(BF)


def r32(g, *s):
    return torch.randn(s, generator=g)


def trunc16(x):
    """a bf16 store that drops the low 16 bits instead of rounding"""
    return (x.float().contiguous().view(torch.int32) & -65536).view(F32).to(BF)


def sig(x):
    return 1.0 / (1.0 + torch.exp(-x))


def silu(x):
    return x * sig(x)


def dsilu(x):
    s = sig(x)
    return s * (1.0 + x * (1.0 - s))


def serial(t, dim=0):
    t = t.movedim(dim, 0)
    acc = torch.zeros_like(t[0])
    for i in range(t.shape[0]):
        acc = acc + t[i]
    return acc


def admit(what, got, ref):
    ratios = ab.judge(got, ref)
    print(f"{what}: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert all(v <= 1.0 for v in ratios.values()), (what, ratios)
    return ratios


def reject(what, got, ref):
    ratios = ab.judge(got, ref)
    print(f"{what} (mutant): " + ", ".join(f"{k} {v:.3g}" for k, v in ratios.items()))
    assert any(v > 1.0 for v in ratios.values()), (what, ratios)


def routing(g, B, N, k):
    idx = torch.stack([torch.randperm(N, generator=g)[:k] for _ in range(B)]).int()
    inv = torch.full((B, N), -1, dtype=torch.int32)
    inv.scatter_(1, idx.long(), torch.arange(k, dtype=torch.int32)[None].expand(B, k).contiguous())
    return idx, inv


# ------------------------------------------------------------------------------------------------------------------ tokens
def test_token_routing_bounds():
    g = gen(1)
    B, N, k, D = 3, 5, 3, 8
    idx, inv = routing(g, B, N, k)
    src, keep = r16(g, B * N, D), torch.tensor([1, 0, 1], dtype=torch.int32)
    want = torch.stack([src.reshape(B, N, D)[b, idx[b].long()] if keep[b] else torch.zeros(k, D, dtype=BF) for b in range(B)]).reshape(B * k, D)
    admit("gather", {"dst": want}, ab.gather_ref(src, idx, keep, B, N, k))
    reject("gather: idx without the b * N offset", {"dst": src[idx.reshape(-1).long()]}, ab.gather_ref(src, idx, None, B, N, k))
    d0, s2 = r16(g, B * N, D), r16(g, B * k, D)
    got = d0.clone().reshape(B, N, D)
    for b in range(B):
        for j in range(k):
            got[b, idx[b, j]] = (got[b, idx[b, j]].float() + s2[b * k + j].float()).to(BF)
    ref = ab.scatter_add_ref(s2, idx, d0, B, N, k)
    admit("scatter_add", {"dst": got.reshape(B * N, D)}, ref)
    mut = d0.clone().reshape(B, N, D)
    for b in range(B):
        for j in range(k):
            mut[b, idx[b, j]] = trunc16(mut[b, idx[b, j]].float() + s2[b * k + j].float())
    reject("scatter_add: truncating store", {"dst": mut.reshape(B * N, D)}, ref)
    xd, mask = r16(g, B * k, D), r32(g, D)
    rr = ab.restore_ref(xd, inv, mask, B, N, k)
    want = torch.stack([xd[b * k + int(inv[b, n])] if inv[b, n] >= 0 else mask.to(BF) for b in range(B) for n in range(N)])
    admit("restore", {"out": want}, rr)
    reject("restore: truncated mask token", {"out": torch.stack([xd[b * k + int(inv[b, n])] if inv[b, n] >= 0 else trunc16(mask)
                                                                   for b in range(B) for n in range(N)])}, rr)


def test_gated_residual_bounds():
    g = gen(2)
    rpm, G, D = 5, 3, 72
    M = rpm * G
    x, t, gate = r16(g, M, D), r16(g, M, D), r16(g, G, D)
    ref = ab.gated_residual_ref(x, t, gate, rpm)
    f = x.float() + gate.float().repeat_interleave(rpm, 0) * t.float()
    admit("gated_residual", {"out": f.to(BF)}, ref)
    reject("gated_residual: truncating store", {"out": trunc16(f)}, ref)
    rows = (torch.arange(M) // (rpm + 1)).clamp_max(G - 1)
    reject("gated_residual: rows_per_mod off by one", {"out": (x.float() + gate.float()[rows] * t.float()).to(BF)}, ref)


def test_ddt_bounds():
    g = gen(3)
    B, N, D = 3, 17, 8
    enc, temb = ab.spread((B * N, D), g, DEV, 10.0), ab.spread((B, D), g, DEV, 5.0, dtype=F32)
    u = enc.float() + temb.repeat_interleave(N, 0)
    admit("ddt_fwd", {"out": silu(silu(u)).to(BF)}, ab.ddt_fwd_ref(enc, temb, N))
    dsz, t0 = r16(g, B * N, D), r32(g, B, D)
    ref = ab.ddt_bwd_ref(dsz, enc, temb, t0, N)
    d = dsz.float() * dsilu(silu(u)) * dsilu(u)
    dt = t0 + serial(d.reshape(B, N, D), 1)
    admit("ddt_bwd", {"denc": d.to(BF), "dtemb": dt}, ref)
    reject("ddt_bwd: row / N with the wrong divisor", {"denc": (dsz.float() * dsilu(silu(enc.float() + temb[(torch.arange(B * N) // (N + 1))]))
                                                                * dsilu(enc.float() + temb[(torch.arange(B * N) // (N + 1))])).to(BF), "dtemb": dt}, ref)
    reject("ddt_bwd: a dropped row of dtemb", {"denc": d.to(BF), "dtemb": t0 + serial(d.reshape(B, N, D)[:, :-1], 1)}, ref)


def test_masked_and_column_sums():
    g = gen(4)
    R, C = 769, 24
    x, o0 = r16(g, R, C) + 0.5, r32(g, C)
    sel = torch.zeros(R, dtype=torch.int32)
    sel[torch.rand(R, generator=g) < 0.5] = -1
    xm = torch.where((sel < 0)[:, None], x.float(), torch.zeros(()))
    admit("masked_colsum", {"out": o0 + serial(xm)}, ab.masked_colsum_ref(x, sel, o0))
    # the deterministic vector form: slabs of rps rows, nr thread rows, pairs of rows first
    depth = ab.colsum_det_depth(R, C, 512 * C, True)
    ref = ab.colsum_ref(x, o0, depth)
    slabs = -(-R // 256)
    rps = -(-R // slabs)
    parts = [serial(x.float()[s * rps:(s + 1) * rps]) for s in range(-(-R // rps))]
    admit(f"colsum_det (depth {depth})", {"out": o0 + serial(torch.stack(parts))}, ref)
    reject("colsum: a dropped tail row", {"out": o0 + serial(x.float()[:-1])}, ref)
    reject("colsum: the previous value lost", {"out": serial(x.float())}, ref)
    G, n = 130, 70
    p0, q0 = r32(g, G, n), r32(g, n)
    admit("reduce_rows", {"out": q0 + serial(p0)}, ab.colsum_ref(p0, q0, G + 1))
    admit("reduce_rows_batched", {"out": q0 + serial(p0)}, ab.colsum_ref(p0, q0, ab.reduce_rows_batched_depth(G)))
    reject("reduce_rows_batched: a dropped row", {"out": q0 + serial(p0[:-1])}, ab.colsum_ref(p0, q0, ab.reduce_rows_batched_depth(G)))
    B, HW = 3, 300
    dy = r16(g, B * HW, C)
    rb = ab.rowbias_bwd_ref(dy, B, HW, C)
    admit("rowbias_bwd", {"de": serial(dy.float().reshape(B, HW, C), 1).to(BF)}, rb)
    reject("rowbias_bwd: truncating store", {"de": trunc16(serial(dy.float().reshape(B, HW, C), 1))}, rb)


# ------------------------------------------------------------------------------------------------------------------ embed
def test_embedding_bounds():
    g = gen(5)
    t = torch.tensor([0.0, 0.5, 1.0, 17.0, 999.0])
    for dim in (2, 256):
        half = dim // 2
        fr = torch.exp(torch.arange(half).float() * torch.tensor(-math.log(10000.0) / half).float())
        a = t[:, None] * fr
        ref = ab.timestep_ref(t, dim, 10000.0)
        admit(f"timestep dim {dim}", {"emb": torch.cat([a.cos(), a.sin()], 1).to(BF)}, ref)
        reject("timestep: cos and sin halves swapped", {"emb": torch.cat([a.sin(), a.cos()], 1).to(BF)}, ref)
    x = r32(g, 2, 3, 8, 12)
    for p, cpp in ((2, True), (4, False)):
        want = fb.patchify_ref(x, p, 3 * p * p + 5, cpp)["tok"][0]
        admit("patchify", {"tok": want.to(BF)}, ab.patchify_ref(x, p, 3 * p * p + 5, cpp))
        reject("patchify: truncating store", {"tok": trunc16(want)}, ab.patchify_ref(x, p, 3 * p * p + 5, cpp))
    tok = fb.patchify_ref(x, 2, 12, False)["tok"][0]
    admit("unpatchify", {"img": x}, ab.unpatchify_ref(tok, 2, 3, 8, 12, 2))
    B, E, n_cls = 7, 8, 11
    e, tab, idx = ab.spread((B, E), g, DEV, dtype=F32), r32(g, n_cls, E), torch.tensor([3, 10, 3, 0, 3, 10, 7])
    v = e + tab[idx]
    admit("cond_fwd", {"emb": v, "act": silu(v).to(BF)}, ab.cond_fwd_ref(e, tab[idx]))
    da, dt0 = r32(g, B, E), r32(g, n_cls, E)
    gg = da * dsilu(v)
    dt = dt0.clone()
    for lab in idx.unique():
        rows = (idx == lab).nonzero()[:, 0]
        dt[lab] = dt0[lab] + serial(gg[rows])
    ref = ab.cond_bwd_ref(da, v, idx, dt0)
    admit("cond_bwd", {"demb": gg, "demb16": gg.to(BF), "dtable": dt}, ref)
    dm = dt.clone()
    dm[3] = dt0[3] + gg[0]  # the first owner forgets the later samples of its label
    reject("cond_bwd: the first owner alone", {"demb": gg, "demb16": gg.to(BF), "dtable": dm}, ref)
    pre, dy = ab.spread((1, 4096), g, DEV), r32(g, 1, 4096)
    xf = pre.float()
    dg = 0.5 * (1 + torch.erf(xf * 0.70710678118654752)) + xf * 0.3989422804014327 * torch.exp(-0.5 * xf * xf)
    admit("gelu_bwd", {"dx": (dy * dg).to(BF)}, ab.gelu_bwd_ref(dy, pre))
    admit("silu_bwd", {"dx": (dy * dsilu(xf)).to(BF)}, ab.silu_bwd_ref(dy, pre))
    reject("silu_bwd: truncating store", {"dx": trunc16(dy * dsilu(xf))}, ab.silu_bwd_ref(dy, pre))
    reject("gelu_bwd: the density term lost", {"dx": (dy * 0.5 * (1 + torch.erf(xf * 0.70710678118654752))).to(BF)}, ab.gelu_bwd_ref(dy, pre))


def _rot(x, cs, sn, rot, inverse=False, swap=False):
    """x [B, n, H, 64] f32"""
    x = x.clone()
    a, b = x[..., 0:rot:2].clone(), x[..., 1:rot:2].clone()
    if swap:
        a, b = b, a
    c, s = cs[None, :, None, :], (-sn if inverse else sn)[None, :, None, :]
    x[..., 0:rot:2] = a * c - b * s
    x[..., 1:rot:2] = a * s + b * c
    return x


def test_heads_bounds():
    g = gen(6)
    B, H, n = 2, 3, 7
    for rot in (32, 64):
        cs, sn = fb.rope_tables(n, rot, g, DEV)
        src = r16(g, B * n, H * 64)
        ref = ab.heads_split_ref(src, cs, sn, B, H, n, rot)
        x4 = src.float().reshape(B, n, H, 64)
        admit(f"heads_split rot {rot}", {"dst": _rot(x4, cs, sn, rot).permute(0, 2, 1, 3).to(BF)}, ref)
        reject("heads_split: a pair of swapped rotary components", {"dst": _rot(x4, cs, sn, rot, swap=True).permute(0, 2, 1, 3).to(BF)}, ref)
        reject("heads_split: the table row of the wrong token", {"dst": _rot(x4, cs.roll(1, 0), sn.roll(1, 0), rot).permute(0, 2, 1, 3).to(BF)}, ref)
        dg, s0 = r16(g, B, H, n, 64), r16(g, B * n, H * 64)
        y = _rot(dg.float().permute(0, 2, 1, 3), cs, sn, rot, inverse=True).reshape(B * n, H * 64)
        admit("heads_merge accumulate", {"src": (y + s0.float()).to(BF)}, ab.heads_merge_ref(dg, s0, cs, sn, B, H, n, rot))
        admit("heads_merge", {"src": y.to(BF)}, ab.heads_merge_ref(dg, None, cs, sn, B, H, n, rot))
        reject("heads_merge: the forward rotation", {"src": _rot(dg.float().permute(0, 2, 1, 3), cs, sn, rot).reshape(B * n, H * 64).to(BF)},
               ab.heads_merge_ref(dg, None, cs, sn, B, H, n, rot))
    src = r16(g, B * n, H * 64)
    admit("heads_split plain", {"dst": src.reshape(B, n, H, 64).permute(0, 2, 1, 3)}, ab.heads_split_ref(src, None, None, B, H, n, 0))


def cosine_inputs(g, M, E):
    p, d = r16(g, M, E), r32(g, M, E)
    p[1] = 0.0
    p[3] *= 2.0**-20
    d[3] *= 2.0**-20
    return p, d


def test_cosine_bounds():
    g = gen(7)
    for E in (8, 520):
        M = 5
        p, d = cosine_inputs(g, M, E)
        pf = p.float()
        s, a, b = serial(pf * d, 1), serial(pf * pf, 1), serial(d * d, 1)
        e2 = torch.tensor(1e-8) * torch.tensor(1e-8)
        cosv = s / torch.sqrt(torch.maximum(a * b, e2))
        ref = ab.cosine_fwd_ref(p, d)
        admit(f"cosine_fwd E {E}", {"cos": cosv, "pn2": a, "dn2": b}, ref)
        reject("cosine_fwd: the clamp left out", {"cos": s / torch.sqrt(a * b).clamp_min(1e-30), "pn2": a, "dn2": b}, ref)
        gdev = torch.tensor([0.37])
        refb = ab.cosine_bwd_ref(p, d, cosv, a, b, -0.2, gdev)
        cl = a * b < e2
        inv = 1.0 / torch.sqrt(torch.maximum(a * b, e2))
        k = torch.where(cl, torch.zeros(()), cosv / a.clamp_min(1e-30))
        gs = torch.tensor(-0.2) * gdev[0]
        admit("cosine_bwd", {"dp": (gs * (d * inv[:, None] - k[:, None] * pf)).to(BF)}, refb)
        reject("cosine_bwd: the clamp ignored", {"dp": (gs * (d * inv[:, None] - (cosv / a.clamp_min(1e-30))[:, None] * pf)).to(BF)}, refb)


# ------------------------------------------------------------------------------------------------------------------ unet
def test_im2col_and_weight_shadows():
    g = gen(8)
    B, H, W, C = 2, 3, 4, 3
    x = r16(g, B * H * W, C)
    rows, ld = B * H * W + 37, 40
    ref = ab.im2col_ref(x, B, H, W, C, rows, ld)
    cols = torch.zeros(rows, ld, dtype=BF)
    x4 = x.reshape(B, H, W, C)

    def fill(shift_tap=None):
        out = cols.clone()
        for b in range(B):
            for y in range(H):
                for xx in range(W):
                    for tap in range(9):
                        yy, xw = y + tap // 3 - 1, xx + tap % 3 - 1 + (1 if tap == shift_tap else 0)
                        if 0 <= yy < H and 0 <= xw < W:
                            out[(b * H + y) * W + xx, tap * C:(tap + 1) * C] = x4[b, yy, xw]
        return out

    admit("im2col", {"cols": fill()}, ref)
    reject("im2col: one tap shifted by a pixel", {"cols": fill(shift_tap=5)}, ref)
    Co, Ci = 3, 8
    w = r32(g, Co, Ci, 3, 3)
    ref = ab.cast_conv_ref(w, 9 * Ci + 8, 9 * Co)
    wf, wd = torch.zeros(Co, 9 * Ci + 8, dtype=BF), torch.zeros(Ci, 9 * Co, dtype=BF)
    wd_norot = wd.clone()
    for co in range(Co):
        for ci in range(Ci):
            for tap in range(9):
                v = w[co, ci, tap // 3, tap % 3].to(BF)
                wf[co, tap * Ci + ci] = v
                wd[ci, (8 - tap) * Co + co] = v
                wd_norot[ci, tap * Co + co] = v
    admit("cast_conv", {"wf": wf, "wd": wd}, ref)
    reject("cast_conv: the 180-degree rotation left out", {"wf": wf, "wd": wd_norot}, ref)
    reject("cast_conv: truncating store", {"wf": trunc16(w.reshape(Co, Ci, 9).permute(0, 2, 1).reshape(Co, 9 * Ci)), "wd": wd},
           ab.cast_conv_ref(w, 9 * Ci, 9 * Co))


def test_fold_bounds():
    g = gen(9)
    Co, Ci = 32, 32
    for n in (1, 7, 17):
        gi, d0 = r32(g, n, 9 * Ci, Co), r32(g, Co, Ci * 9)
        ref = ab.fold_ref(gi, d0, Co, Ci)
        t = gi.reshape(n, 9, Ci, Co).permute(0, 3, 2, 1)
        admit(f"fold n_img {n}", {"dw": d0.reshape(Co, Ci, 9) + serial(t)}, ref)
        if n > 1:
            reject("fold: image 0 twice, the last omitted", {"dw": d0.reshape(Co, Ci, 9) + serial(torch.cat([t[:1], t[:-1]]))}, ref)
        reject("fold: the previous value lost", {"dw": serial(t)}, ref)


def test_resample_glu_and_glue_bounds():
    g = gen(10)
    B, Hs, Ws, C = 2, 3, 5, 24
    xb, xs = r16(g, B * 4 * Hs * Ws, C), r16(g, B * Hs * Ws, C)
    t6 = xb.float().reshape(B, Hs, 2, Ws, 2, C)
    for scale in (1.0, 0.25):
        f = scale * (t6[:, :, 0, :, 0] + t6[:, :, 0, :, 1] + t6[:, :, 1, :, 0] + t6[:, :, 1, :, 1])
        ref = ab.reduce2x2_ref(xb, B, Hs, Ws, C, scale)
        admit(f"reduce2x2 {scale}", {"out": f.reshape(-1, C).to(BF)}, ref)
        reject("reduce2x2: truncating store", {"out": trunc16(f.reshape(-1, C))}, ref)
        up = (scale * xs.float().reshape(B, Hs, 1, Ws, 1, C).expand(B, Hs, 2, Ws, 2, C)).reshape(-1, C).to(BF)
        admit(f"expand2x2 {scale}", {"out": up}, ab.expand2x2_ref(xs, B, Hs, Ws, C, scale))
    admit("pick", {"out": xb.reshape(B, Hs, 2, Ws, 2, C)[:, :, 0, :, 0].reshape(-1, C)}, ab.pick_ref(xb, B, Hs, Ws, C))
    reject("pick: the odd column", {"out": xb.reshape(B, Hs, 2, Ws, 2, C)[:, :, 0, :, 1].reshape(-1, C)}, ab.pick_ref(xb, B, Hs, Ws, C))
    st = torch.zeros(B, Hs, 2, Ws, 2, C, dtype=BF)
    st[:, :, 0, :, 0] = xs.reshape(B, Hs, Ws, C)
    admit("stuff", {"out": st.reshape(-1, C)}, ab.stuff_ref(xs, B, Hs, Ws, C))
    e = r16(g, B, C)
    f = xs.float().reshape(B, Hs * Ws, C) + e.float()[:, None]
    admit("rowbias_add", {"out": f.reshape(-1, C).to(BF)}, ab.rowbias_add_ref(xs, e, B, Hs * Ws, C))
    reject("rowbias_add: the bias row of the wrong sample", {"out": (xs.float().reshape(B, Hs * Ws, C) + e.float().flip(0)[:, None]).reshape(-1, C).to(BF)},
           ab.rowbias_add_ref(xs, e, B, Hs * Ws, C))
    M, F = 33, 264
    u, dh = ab.spread((M, 2 * F), g, DEV), r16(g, M, F)
    af, gf, df = u[:, :F].float(), u[:, F:].float(), dh.float()
    ge = 0.5 * gf * (1 + torch.erf(gf * 0.70710678118654752))
    dge = 0.5 * (1 + torch.erf(gf * 0.70710678118654752)) + gf * 0.39894228040143268 * torch.exp(-0.5 * gf * gf)
    admit("geglu_fwd", {"h": (af * ge).to(BF)}, ab.geglu_fwd_ref(u, F))
    admit("geglu_bwd", {"du": torch.cat([df * ge, df * af * dge], 1).to(BF)}, ab.geglu_bwd_ref(dh, u, F))
    reject("geglu_bwd: the halves swapped", {"du": torch.cat([df * af * dge, df * ge], 1).to(BF)}, ab.geglu_bwd_ref(dh, u, F))
    admit("swiglu_fwd", {"h": (silu(af) * gf).to(BF)}, ab.swiglu_fwd_ref(u, F))
    reject("swiglu_fwd: truncating store", {"h": trunc16(silu(af) * gf)}, ab.swiglu_fwd_ref(u, F))
    admit("swiglu_bwd", {"du": torch.cat([df * gf * dsilu(af), df * silu(af)], 1).to(BF)}, ab.swiglu_bwd_ref(dh, u, F))
    a, b = r16(g, 7, 24, scale=4.0), r16(g, 7, 24)
    admit("add_bf16", {"out": (a.float() + b.float()).to(BF)}, ab.add_ref(a, b))
    reject("add_bf16: truncating store", {"out": trunc16(a.float() + b.float())}, ab.add_ref(a, b))


# ------------------------------------------------------------------------------------------------------------------ generators, tables
def test_fast_exp_allowances_follow_the_table():
    assert ab.FAST_EXP_ABS == math.ceil(2 * 0.8992) and ab.FAST_EXP_ABS <= fb.ULP_CAP
    assert ab.FAST_EXP_ULP == {4: math.ceil(2 * 4.0258), 8: math.ceil(2 * 7.6843), 16: math.ceil(2 * 15.0879)}
    # past the cap as relative allowances: they reach an output only under s (1 - s) -- at most 2.1 ulp of 1 in the sigmoid
    x = torch.linspace(-16, 16, 100001, dtype=torch.float64)
    s = torch.sigmoid(x)
    ulps = torch.where(x.abs() <= 4, 9.0, torch.where(x.abs() <= 8, 16.0, 31.0))
    assert float((s * (1 - s) * ulps).max()) <= 2.25
    with pytest.raises(AssertionError):
        ab.fast_exp_(fb.V(torch.tensor([17.0], dtype=torch.float64)))


def test_generators_give_finite_references():
    g = gen(11)
    for lim in (5.0, 10.0, 12.0):
        for dt in (BF, F32):
            t = ab.spread((33, 16), g, DEV, lim, dtype=dt)
            assert bool(torch.isfinite(t.float()).all()) and float(t.float().abs().max()) <= lim
    enc, temb = ab.spread((6, 8), g, DEV, 10.0), ab.spread((2, 8), g, DEV, 5.0, dtype=F32)
    refs = [ab.ddt_fwd_ref(enc, temb, 3), ab.ddt_bwd_ref(r16(g, 6, 8), enc, temb, r32(g, 2, 8), 3),
            ab.gelu_bwd_ref(r32(g, 1, 64), ab.spread((1, 64), g, DEV)), ab.silu_bwd_ref(r32(g, 1, 64), ab.spread((1, 64), g, DEV)),
            ab.geglu_bwd_ref(r16(g, 4, 8), ab.spread((4, 16), g, DEV), 8), ab.swiglu_bwd_ref(r16(g, 4, 8), ab.spread((4, 16), g, DEV), 8),
            ab.timestep_ref(torch.tensor([0.0, 0.5, 1.0, 17.0, 999.0]), 256, 10000.0),
            ab.cosine_fwd_ref(*cosine_inputs(g, 5, 512))]
    for ref in refs:
        for name, (r, bound) in ref.items():
            assert bool(torch.isfinite(r.double()).all()), name
            assert bound is None or bool(torch.isfinite(bound).all()), name


def test_entry_points_and_coverage_agree():
    assert set(ab.ENTRY_POINTS) == set(ab.COVERAGE)
