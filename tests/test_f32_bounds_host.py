"""What the fp32-regime bounds of tests/f32_bounds.py admit and what they reject (no GPU).

A torch-f32 emulation of each kernel's arithmetic in the kernel's own order must stay inside every bound on the input classes of the
GPU table (tests/test_f32_paths_gpu.py):
    row kernels   a lane adds its float4 chunks in order, (v0 + v1) + (v2 + v3) inside a chunk, then the 6-level wave tree
    GEMM          one fmaf per k in order (the f32 MFMA), per K-chunk of a split, partial images folded in order
    GroupNorm     thread t walks elements t, t + 256, ...; wave tree; (w0 + w1) + (w2 + w3)
    the rest      element-wise steps in the kernels' order, serial sums where the kernel fixes one writer
Planted mutants must each leave at least one bound or bit-compare (MUTANTS below); the report of which output caught each is printed.
The fp64 references are checked against torch's fp64 autograd, and the coverage list against the header.
"""

from __future__ import annotations

import os
import re

import pytest
import torch
import torch.nn.functional as Fn

import f32_bounds as fb
import groupnorm_bounds as gb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT: dict[str, tuple[float, str]] = {}
F32 = torch.float32


def note(fam, ratios, where):
    for k, v in ratios.items():
        if v > REPORT.get(f"{fam}.{k}", (-1.0, ""))[0]:
            REPORT[f"{fam}.{k}"] = (v, where)


def inside(fam, got, ref, where):
    r = fb.judge(got, ref)
    note(fam, r, where)
    assert all(v <= 1.0 for v in r.values()), f"{fam} {where}: {r}"
    return r


# ------------------------------------------------------------------------------------------------------------------ shared pieces
def tree(v):
    """[.., 64] lanes -> the wave sum: six pairwise levels in lane order"""
    while v.shape[-1] > 1:
        v = v[..., 0::2] + v[..., 1::2]
    return v[..., 0]


def fr_sum(v, drop_j1=False):
    """v f32 [M, D] (D % 4 == 0, <= 1024) -> [M]: fr_sum of csrc/f32.hip"""
    M, D = v.shape
    c = Fn.pad(v, (0, 1024 - D)).reshape(M, 4, 64, 4)  # [row, chunk j, lane, element]
    q = (c[..., 0] + c[..., 1]) + (c[..., 2] + c[..., 3])
    s = torch.zeros(M, 64)
    for j in range(4):
        if not (drop_j1 and j == 1):
            s = s + q[:, j]
    return tree(s)


def silu32(x):
    return x / (1.0 + torch.exp(-x))


def dsilu32(x):
    s = 1.0 / (1.0 + torch.exp(-x))
    return s * (1.0 + x * (1.0 - s))


def serial(t, dim):
    """sum over `dim` one term after the other"""
    t = t.movedim(dim, 0)
    acc = torch.zeros_like(t[0])
    for i in range(t.shape[0]):
        acc = acc + t[i]
    return acc


def lanes_then(t, lanes, combine):
    """t [n, ..]: lane l adds terms l, l + lanes, ... in order; combine: 'serial' over the lanes or 'pairs' ((l0 + l1) + (l2 + l3) ...)"""
    n = t.shape[0]
    T = -(-n // lanes)
    t = torch.cat([t, torch.zeros(T * lanes - n, *t.shape[1:])]).reshape(T, lanes, *t.shape[1:])
    acc = serial(t, 0)
    if combine == "serial":
        return serial(acc, 0)
    while acc.shape[0] > 1:
        acc = acc[0::2] + acc[1::2]
    return acc[0]


# ------------------------------------------------------------------------------------------------------------------ LayerNorm + modulate
def emu_ln_fwd(x, w, b, scale, shift, rpm, eps, t=None, gate=None, mut=""):
    M, D = x.shape
    res = {}
    live = torch.ones(D, dtype=torch.bool)
    if mut == "drop_j1":
        live[256:512] = False  # chunk j = 1 of every lane never loaded
    xv = x
    if t is not None:
        xv = x + t * fb._rows_mod(gate, rpm, M)
        res["x_out"] = xv
    xv = torch.where(live[None], xv, torch.zeros(1))
    n_mean = 4 * -(-(D // 4) // 64) * 64 if mut == "mean_n" else D
    invD = torch.tensor(1.0) / torch.tensor(float(n_mean))
    mu = fr_sum(xv) * invD
    d = torch.where(live[None], xv - mu[:, None], torch.zeros(1))
    rs = 1.0 / torch.sqrt(fr_sum(d * d) * invD + torch.tensor(eps, dtype=F32))
    y = d * rs[:, None]
    if w is not None:
        y = y * w + b
    sc, sh = fb._rows_mod(scale, rpm, M), fb._rows_mod(shift, rpm, M)
    res.update(out=y * ((0.0 if mut == "scale_no1" else 1.0) + sc) + sh, mean=mu, rstd=rs)
    return res


def emu_ln_bwd(dout, x, w, b, scale, rpm, mean, rstd, dres=None, want_dwb=False, gate_t=None, gate=None, mut=""):
    M, D = x.shape
    G = M // rpm
    invD = torch.tensor(1.0) / torch.tensor(float(D))
    sc = fb._rows_mod(scale, rpm, M)
    xh = (x - mean[:, None]) * rstd[:, None]
    dy = dout * (1.0 + sc)
    if w is not None:
        dy = dy * w
    m1, m2 = fr_sum(dy) * invD, fr_sum(dy * xh) * invD
    r = (dy - m1[:, None] - xh * m2[:, None]) * rstd[:, None]
    if dres is not None and mut != "dres":
        r = dres + r
    res = {"dx": r}
    grp = lambda v: lanes_then(v.reshape(G, rpm, D).movedim(1, 0), 8, "serial")  # noqa: E731
    a1, a2 = grp(dout), grp(dout * xh)
    res["dscale"] = (w * a2 + b * a1) if w is not None else a2
    res["dshift"] = a1
    if want_dwb:
        s1 = 1.0 + scale
        res["dwb"] = torch.stack([s1 * a2, s1 * a1], 1)
    if gate_t is not None:
        res["dt"] = r * fb._rows_mod(gate, rpm, M)
        res["dgate"] = grp(r * gate_t)
    return res


def ln_inputs(D, rpm, G, cls, flags, seed=0):
    g = torch.Generator().manual_seed(seed + D)
    n = lambda *s: torch.randn(s, generator=g)  # noqa: E731
    M = rpm * G
    x = fb.row_input(cls, M, D, g, "cpu")
    w, b = (1.0 + 0.2 * n(D), 0.2 * n(D)) if "w" in flags else (None, None)
    mod = 0.3 * n(G, 6 * D)
    t = n(M, D) if "g" in flags else None
    return dict(x=x, w=w, b=b, shift=mod[:, :D], scale=mod[:, D:2 * D], gate=mod[:, 2 * D:3 * D] if t is not None else None, t=t,
                dout=n(M, D), dres=n(M, D) if "r" in flags else None, rpm=rpm)


def ln_ratios(D, rpm, G, cls, flags, mut=""):
    i = ln_inputs(D, rpm, G, cls, flags)
    ref = fb.ln_fwd_ref(i["x"], i["w"], i["b"], i["scale"], i["shift"], rpm, fb.LN_EPS, i["t"], i["gate"])
    got = emu_ln_fwd(i["x"], i["w"], i["b"], i["scale"], i["shift"], rpm, fb.LN_EPS, i["t"], i["gate"], mut)
    r = fb.judge(got, ref)
    # the backward takes CORRECT f32 statistics: a mutant of the backward is judged on the backward's own outputs
    xin = ref["x_out"][0].float() if i["t"] is not None else i["x"]
    mean, rstd = ref["mean"][0].float(), ref["rstd"][0].float()
    a = (i["dout"], xin, i["w"], i["b"], i["scale"], rpm, mean, rstd, i["dres"], "p" in flags and i["w"] is not None, i["t"], i["gate"])
    r.update(fb.judge(emu_ln_bwd(*a, mut=mut), fb.ln_bwd_ref(*a)))
    return r


LN_TABLE = [(4, 13, 3, "scaled", "wgrp"), (252, 13, 3, "offset32", ""), (256, 13, 3, "const", "wr"), (260, 13, 3, "scaled", "g"),
            (384, 13, 3, "offset32", "wp"), (1020, 13, 3, "const", "gr"), (1024, 13, 3, "scaled", "wg"), (260, 1, 5, "offset32", "wgrp"),
            (1024, 13, 3, "const", "wgrp"), (260, 13, 3, "const", "")]


@pytest.mark.parametrize("D,rpm,G,cls,flags", LN_TABLE)
def test_ln_emulation_inside_bounds(D, rpm, G, cls, flags):
    r = ln_ratios(D, rpm, G, cls, flags)
    note("ln", r, f"D{D} {cls} {flags}")
    assert all(v <= 1.0 for v in r.values()), r


# ------------------------------------------------------------------------------------------------------------------ QK-RMSNorm + RoPE
def _rot_emu(y, cs, sn, tok, H, dh, rot, inverse, rot_all=False):
    M, D = y.shape
    if rot == 0:
        return y
    half = rot // 2
    ch = torch.arange(dh)
    on = (ch < (dh if rot_all else rot)).repeat(H)
    pair = ((ch // 2) % half).repeat(H)
    c, s = cs[tok][:, pair], sn[tok][:, pair]
    yp = fb._swap_pairs(y)
    even = (torch.arange(D) % 2 == 0)[None]
    if inverse:
        r = torch.where(even, y * c + yp * s, -yp * s + y * c)
    else:
        r = torch.where(even, y * c - yp * s, yp * s + y * c)
    return torch.where(on[None], r, y)


def emu_qk_fwd(qkv, sq, sk, cs, sn, tok, H, dh, rot, eps, mut=""):
    M, D = qkv.shape[0], H * dh
    invD = torch.tensor(1.0) / torch.tensor(float(D))
    if mut == "pos_ignored":
        tok = torch.arange(M) % 13
    qs, rs = [], []
    for part, scl in ((0, sq), (1, sk)):
        v = qkv[:, part * D:(part + 1) * D]
        r = 1.0 / torch.sqrt(fr_sum(v * v) * invD + torch.tensor(eps, dtype=F32))
        qs.append(_rot_emu(v * r[:, None] * scl, cs, sn, tok, H, dh, rot, False, mut == "rot_all"))
        rs.append(r)
    return {"qk": torch.cat(qs, 1), "rrms": torch.stack(rs, 1)}


def emu_qk_bwd(dqk, qkv, sq, sk, cs, sn, tok, rrms, B, N, H, dh, rot, mut=""):
    M, D = qkv.shape[0], H * dh
    invD = torch.tensor(1.0) / torch.tensor(float(D))
    dxs, dss = [], []
    for part, scl in ((0, sq), (1, sk)):
        g = _rot_emu(dqk[:, part * D:(part + 1) * D], cs, sn, tok, H, dh, rot, mut != "inv_sign")
        x, r = qkv[:, part * D:(part + 1) * D], rrms[:, part:part + 1]
        dss.append(lanes_then((g * x * r).reshape(B, N, D).movedim(1, 0), 4, "pairs"))
        gx = g * scl
        m = fr_sum(gx * x) * invD
        dxs.append(r * (gx - x * (r * r * m[:, None])))
    return {"dqk_in": torch.cat(dxs, 1), "dscale": torch.stack(dss, 1)}


def qk_ratios(H, dh, rot, use_pos, mut=""):
    B, N, D = 2, 13, H * dh
    g = torch.Generator().manual_seed(H * 1000 + dh + rot)
    n = lambda *s: torch.randn(s, generator=g)  # noqa: E731
    qkv = n(B * N, 3 * D) * (0.5 + torch.rand(1, 3 * D, generator=g))
    sq, sk = 1.0 + 0.2 * n(D), 1.0 + 0.2 * n(D)
    cs, sn = fb.rope_tables(19, rot, g, "cpu")
    tok = torch.randint(0, 19, (B * N,), generator=g) if use_pos else torch.arange(B * N) % N
    ref = fb.qk_fwd_ref(qkv, sq, sk, cs, sn, tok, H, dh, rot, fb.QK_EPS)
    r = fb.judge(emu_qk_fwd(qkv, sq, sk, cs, sn, tok, H, dh, rot, fb.QK_EPS, mut), ref)
    dqk, rr = n(B * N, 2 * D), ref["rrms"][0].float()
    r.update(fb.judge(emu_qk_bwd(dqk, qkv, sq, sk, cs, sn, tok, rr, B, N, H, dh, rot, mut),
                      fb.qk_bwd_ref(dqk, qkv, sq, sk, cs, sn, tok, rr, B, N, H, dh, rot)))
    return r


@pytest.mark.parametrize("H,dh", [(1, 4), (2, 64), (6, 64), (16, 64), (3, 84)])
def test_qk_emulation_inside_bounds(H, dh):
    for j, rot in enumerate(sorted({0, (dh // 2 + 3) // 4 * 4, dh})):
        r = qk_ratios(H, dh, rot, j % 2 == 0)
        note("qk", r, f"H{H} dh{dh} rot{rot}")
        assert all(v <= 1.0 for v in r.values()), (rot, r)


# ------------------------------------------------------------------------------------------------------------------ GEMM
def split_plan(M, N, K, scratch_floats):
    """(splits, kchunk) as dl_f32_gemm picks them for an unbatched product"""
    tiles = -(-M // 128) * -(-N // 128)
    splits, kchunk = 1, -(-K // 16) * 16
    if scratch_floats and tiles < 768 and K >= 1024:
        want = min(-(-1024 // tiles), K // 256, scratch_floats // (M * N), 64)
        if want >= 2:
            kchunk = -(-(-(-K // want)) // 16) * 16
            splits = -(-K // kchunk)
    return splits, kchunk


def fma_chain(a, b, k0, k1):
    """sum_k a[:, k] b[:, k] as one fmaf per k in order (fp64 product and sum, rounded to f32 each step)"""
    acc = torch.zeros(a.shape[0], b.shape[0])
    A, B = a.double(), b.double()
    for k in range(k0, k1):
        acc = (A[:, k:k + 1] * B[None, :, k] + acc.double()).float()
    return acc


def emu_gemm(a, b, alpha, bias, silu, c0, want_pre, scratch_floats, mut=""):
    M, K = a.shape
    N = b.shape[0]
    splits, kchunk = split_plan(M, N, K, scratch_floats)
    parts = [fma_chain(a, b, s * kchunk, min((s + 1) * kchunk, K)) for s in range(splits)]
    if mut == "bias_per_split" and bias is not None:
        parts = [p + bias for p in parts]
    if mut == "drop_last_split":
        parts = parts[:-1]
    s = parts[0]
    for p in parts[1:]:
        s = s + p
    v = torch.tensor(alpha, dtype=F32) * s
    if bias is not None and mut != "bias_per_split":
        v = v + bias
    res = {}
    if want_pre:
        res["pre_out"] = silu32(v) if mut == "silu_before_pre" else v
    if silu:
        v = silu32(v)
    if c0 is not None:
        v = v + c0
    res["C"] = v
    return res


def gemm_ratios(M, N, K, alpha=1.0, bias=False, silu=False, acc=False, pre=False, scratch=0, mut=""):
    g = torch.Generator().manual_seed(M * 7 + N * 3 + K)
    n = lambda *s: torch.randn(s, generator=g)  # noqa: E731
    a, b = n(M, K), n(N, K)
    bv, c0 = (n(N) if bias else None), (n(M, N) if acc else None)
    ref = fb.gemm_ref(a, b, alpha, bv, silu, c0, pre)
    return fb.judge(emu_gemm(a, b, alpha, bv, silu, c0, pre, scratch, mut), ref)


GEMM_TABLE = [dict(M=1, N=1, K=1), dict(M=128, N=128, K=16), dict(M=129, N=127, K=17), dict(M=132, N=124, K=20, alpha=0.37, bias=True),
              dict(M=132, N=124, K=20, bias=True, silu=True, pre=True), dict(M=132, N=124, K=20, acc=True, alpha=-1.5, bias=True),
              dict(M=260, N=36, K=1028), dict(M=260, N=36, K=1040, scratch=64 * 260 * 36), dict(M=129, N=127, K=2050, scratch=2 * 129 * 127, bias=True),
              dict(M=132, N=124, K=1040, scratch=64 * 132 * 124, bias=True, silu=True, pre=True),
              dict(M=132, N=124, K=1040, scratch=64 * 132 * 124, acc=True, alpha=-1.5, bias=True)]


@pytest.mark.parametrize("kw", GEMM_TABLE, ids=[f"{k['M']}x{k['N']}x{k['K']}-{i}" for i, k in enumerate(GEMM_TABLE)])
def test_gemm_emulation_inside_bounds(kw):
    r = gemm_ratios(**kw)
    note("gemm", r, str(kw))
    assert all(v <= 1.0 for v in r.values()), r


def test_split_plan_matches_the_table():
    """the splits the GPU table was written for: four of 272 (last 224), two images -> two splits, below two images -> none"""
    assert split_plan(260, 36, 1040, 64 * 260 * 36) == (4, 272)
    assert split_plan(132, 124, 1040, 2 * 132 * 124) == (2, 528)
    assert split_plan(132, 124, 1040, 2 * 132 * 124 - 1) == (1, 1040)
    assert split_plan(260, 36, 2050, 64 * 260 * 36)[0] > 1 and split_plan(260, 36, 1028, 0)[0] == 1


# ------------------------------------------------------------------------------------------------------------------ softmax
def scores(rows, cols, g):
    """the rows of the GPU table: a +80 spike on the row maximum, some -inf, -1e4 throughout"""
    s = 3.0 * torch.randn(rows, cols, generator=g)
    s[0, s[0].argmax()] += 80.0
    s[1, ::3] = float("-inf")
    s[1, 1 % cols] = 0.5
    s[2] = -1.0e4
    return s


def _lane_sum(e, cols, vec):
    rows = e.shape[0]
    if vec:
        c = Fn.pad(e, (0, 4096 - cols)).reshape(rows, 16, 64, 4)
        q = (c[..., 0] + c[..., 1]) + (c[..., 2] + c[..., 3])
        return tree(serial(q, 1))
    T = -(-cols // 64)
    return tree(serial(Fn.pad(e, (0, T * 64 - cols)).reshape(rows, T, 64), 1))


def emu_softmax_fwd(s, vec, bias=None, mut=""):
    rows, cols = s.shape
    z = s if bias is None else s + bias
    mx = z.max(-1, keepdim=True).values
    dead = mx == float("-inf")
    if mut == "nomax":
        mx = torch.zeros_like(mx)
    e = torch.exp(z - torch.where(dead, torch.zeros_like(mx), mx))
    p = e * (1.0 / _lane_sum(e, cols, vec))[:, None]
    if bias is not None and mut != "masked_nan":
        p = torch.where(dead, torch.zeros_like(p), p)
    return {"p": p}


def emu_softmax_bwd(p, dp, vec):
    dot = _lane_sum(p * dp, p.shape[1], vec)
    return {"ds": p * (dp - dot[:, None])}


def softmax_ratios(cols, mut=""):
    g = torch.Generator().manual_seed(cols)
    s = scores(7, cols, g)
    vec = cols % 4 == 0 and cols <= 4096
    r = fb.judge(emu_softmax_fwd(s, vec, mut=mut), fb.softmax_fwd_ref(s, vec))
    p, dp = torch.softmax(s.double(), -1).float(), torch.randn(7, cols, generator=g)
    r.update(fb.judge(emu_softmax_bwd(p, dp, vec), fb.softmax_bwd_ref(p, dp, vec)))
    return r


@pytest.mark.parametrize("cols", [1, 3, 4, 9, 25, 252, 256, 260, 4092, 4096, 4100])
def test_softmax_emulation_inside_bounds(cols):
    r = softmax_ratios(cols)
    note("softmax", r, f"cols {cols}")
    assert all(v <= 1.0 for v in r.values()), r


def keymask_ratios(mut=""):
    B, rps, cols = 3, 5, 77
    g = torch.Generator().manual_seed(77)
    s = 3.0 * torch.randn(B * rps, cols, generator=g)
    bias = torch.zeros(B, cols)
    bias[0] = float("-inf")
    bias[1, 40:] = float("-inf")
    kb = bias.repeat_interleave(rps, 0)
    return fb.judge(emu_softmax_fwd(s, False, kb, mut), fb.softmax_fwd_ref(s, False, kb))


def test_keymask_emulation_inside_bounds():
    inside("keymask", emu_softmax_fwd(torch.zeros(2, 5), False, torch.zeros(2, 5)), fb.softmax_fwd_ref(torch.zeros(2, 5), False, torch.zeros(2, 5)), "zeros")
    r = keymask_ratios()
    note("keymask", r, "B3 rps5 cols77")
    assert all(v <= 1.0 for v in r.values()), r


# ------------------------------------------------------------------------------------------------------------------ elementwise and routing
def test_elementwise_emulations_inside_bounds():
    g = torch.Generator().manual_seed(3)
    n = lambda *s: torch.randn(s, generator=g)  # noqa: E731
    for F in (4, 96, 100, 3):
        u = 2.0 * n(7, 2 * F)
        for half in (u[:, :F], u[:, F:]):
            half[0, 0], half[1, 0], half[2, 0] = 30.0, -30.0, 0.0
        a, gg, dh = u[:, :F], u[:, F:], n(7, F)
        c1, c2 = torch.tensor(fb.INV_SQRT2, dtype=F32), torch.tensor(fb.INV_SQRT2PI, dtype=F32)
        inside("geglu_fwd", {"h": a * (0.5 * gg * (1.0 + torch.erf(gg * c1)))}, fb.geglu_fwd_ref(u, F), f"F{F}")
        cdf = 0.5 * (1.0 + torch.erf(gg * c1))
        du = torch.cat([dh * gg * cdf, dh * a * (cdf + gg * c2 * torch.exp(-0.5 * gg * gg))], 1)
        inside("geglu_bwd", {"du": du}, fb.geglu_bwd_ref(dh, u, F), f"F{F}")
        inside("swiglu_fwd", {"h": silu32(a) * gg}, fb.swiglu_fwd_ref(u, F), f"F{F}")
        inside("swiglu_bwd", {"du": torch.cat([dh * gg * dsilu32(a), dh * silu32(a)], 1)}, fb.swiglu_bwd_ref(dh, u, F), f"F{F}")
        inside("add", {"out": a + gg}, fb.add_ref(a, gg), f"F{F}")
        inside("silu_bwd", {"dx": dh * dsilu32(a)}, fb.silu_bwd_ref(dh, a), f"F{F}")
    # gates, DDT conditioning, routing
    for D in (4, 260, 1024):
        for rpm, G in ((1, 5), (13, 2)):
            M = rpm * G
            x, t, dout, gate = n(M, D), n(M, D), n(M, D), n(G, D)
            gm = fb._rows_mod(gate, rpm, M)
            inside("gated_residual", {"out": x + gm * t}, fb.gated_residual_ref(x, t, gate, rpm), f"D{D}")
            dg = lanes_then((dout * t).reshape(G, rpm, D).movedim(1, 0), 8, "pairs")
            inside("gate_bwd", {"dt": dout * gm, "dgate": dg}, fb.gate_bwd_ref(dout, t, gate, rpm), f"D{D}")
            enc, temb = 2.0 * n(M, D), 2.0 * n(G, D)
            enc[0, :3], temb[0, :3] = torch.tensor([30.0, -30.0, 0.0]), 0.0
            uu = enc + temb.repeat_interleave(rpm, 0)
            inside("ddt_fwd", {"out": silu32(silu32(uu))}, fb.ddt_fwd_ref(enc, temb, rpm), f"D{D}")
            de = dout * dsilu32(silu32(uu)) * dsilu32(uu)
            inside("ddt_bwd", {"denc": de, "dtemb": lanes_then(de.reshape(G, rpm, D).movedim(1, 0), 8, "pairs")}, fb.ddt_bwd_ref(dout, enc, temb, rpm), f"D{D}")
        x, sel = n(45, D) + 1.0, torch.zeros(45, dtype=torch.int32)
        sel[torch.rand(45, generator=g) < 0.5] = -1
        xm = torch.where((sel < 0)[:, None], x, torch.zeros(1))
        part = torch.stack([lanes_then(xm[s * 15:(s + 1) * 15], 4, "pairs") for s in range(3)])
        inside("colsum", {"part": part}, fb.colsum_ref(x, sel, 3), f"C{D}")
        idx = torch.stack([torch.randperm(13, generator=g)[:5] for _ in range(2)]).int()
        src, d0 = n(10, D), n(26, D)
        dst = d0.clone().reshape(2, 13, D)
        for bb in range(2):
            dst[bb, idx[bb].long()] += src.reshape(2, 5, D)[bb]
        inside("scatter", {"dst": dst.reshape(26, D)}, fb.scatter_add_ref(src, idx, d0, 2, 13, 5), f"D{D}")
    # timestep embedding, cond-combine
    t = torch.tensor([0.0, 0.5, 999.0, 250.25, 1000.0])
    for dim in (2, 64, 65):
        half = dim // 2
        k = torch.arange(half, dtype=F32)
        f = torch.exp(k * torch.tensor(-9.210340371976184, dtype=F32) / torch.tensor(float(half)))
        a = t[:, None] * f[None]
        inside("timestep", {"emb": torch.cat([torch.cos(a), torch.sin(a), torch.zeros(5, dim - 2 * half)], 1)}, fb.timestep_ref(t, dim, 10000.0), f"dim{dim}")
    idx = torch.tensor([1, 4, 1, 0, 4, 1, 3])
    e, table, dact, dt0 = 3.0 * n(7, 100), n(5, 100), n(7, 100), n(5, 100)
    emb = e + table[idx]
    inside("cond_fwd", {"emb": emb, "act": silu32(emb)}, fb.cond_fwd_ref(e, table, idx), "E100")
    demb, dtab = dact * dsilu32(emb), dt0.clone()
    for bb in range(7):
        dtab[idx[bb]] = dtab[idx[bb]] + demb[bb]
    inside("cond_bwd", {"demb": demb, "dtable": dtab}, fb.cond_bwd_ref(dact, emb, idx, dt0), "E100")


# ------------------------------------------------------------------------------------------------------------------ UNet
def emu_im2col(x, B, H, W, C, mut=""):
    x4 = x.reshape(B, H, W, C)
    cols = torch.zeros(B, H, W, C, 9)
    Hb, Wb = (W, H) if mut == "hw_swap" else (H, W)  # the border test
    for tap in range(9):
        for yy in range(H):
            for xx in range(W):
                y2, x2 = yy + tap // 3 - 1, xx + tap % 3 - 1
                if 0 <= y2 < Hb and 0 <= x2 < Wb:
                    cols[:, yy, xx, :, tap] = x4[:, min(y2, H - 1), min(x2, W - 1), :]
    return {"cols": cols.reshape(B * H * W, C * 9)}


def emu_col2im(dcols, B, H, W, C, mut=""):
    d = dcols.reshape(B, H, W, C, 9)
    dx = torch.zeros(B, H, W, C)
    sgn = 1 if mut == "unmirrored" else -1
    for yy in range(H):
        for xx in range(W):
            s = torch.zeros(B, C)
            for tap in range(9):
                y2, x2 = yy + sgn * (tap // 3 - 1), xx + sgn * (tap % 3 - 1)
                if 0 <= y2 < H and 0 <= x2 < W:
                    s = s + d[:, y2, x2, :, tap]
            dx[:, yy, xx] = s
    return {"dx": dx.reshape(B * H * W, C)}


def emu_resample(x, B, Hs, Ws, C, scale, mode, mut=""):
    sc = torch.tensor(scale, dtype=F32)
    if mode == 0:
        t = x.reshape(B, Hs, 2, Ws, 2, C)
        top = t[:, :, 0, :, 0] + t[:, :, 0, :, 1]
        o = sc * (top if mut == "sum2of4" else top + (t[:, :, 1, :, 0] + t[:, :, 1, :, 1]))
        return {"out": o.reshape(B * Hs * Ws, C)}
    if mode == 1:
        return {"out": (sc * x.reshape(B, Hs, 1, Ws, 1, C)).expand(B, Hs, 2, Ws, 2, C).reshape(B * 4 * Hs * Ws, C)}
    if mode == 2:
        return {"out": x.reshape(B, 2 * Hs, 2 * Ws, C)[:, ::2, ::2].reshape(B * Hs * Ws, C)}
    o = torch.zeros(B, 2 * Hs, 2 * Ws, C)
    o[:, ::2, ::2] = x.reshape(B, Hs, Ws, C)
    return {"out": o.reshape(B * 4 * Hs * Ws, C)}


IMG = [(1, 1, 1, 1), (2, 1, 5, 3), (2, 5, 1, 3), (2, 6, 10, 5), (3, 4, 4, 48)]


def img_ratios(B, H, W, C, mut=""):
    g = torch.Generator().manual_seed(H * 100 + W)
    n = lambda *s: torch.randn(s, generator=g)  # noqa: E731
    P = B * H * W
    x, dcols, big = n(P, C), n(P, C * 9), n(4 * P, C)
    r = {"im2col": fb.judge(emu_im2col(x, B, H, W, C, mut), fb.im2col_ref(x, B, H, W, C))["cols"],
         "col2im": fb.judge(emu_col2im(dcols, B, H, W, C, mut), fb.col2im_ref(dcols, B, H, W, C))["dx"]}
    for mode, src in ((0, big), (1, x), (2, big), (3, x)):
        r[f"resample{mode}"] = fb.judge(emu_resample(src, B, H, W, C, 0.25, mode, mut), fb.resample_ref(src, B, H, W, C, 0.25, mode))["out"]
    e = n(B, C)
    r["rowbias_add"] = fb.judge({"out": (x.reshape(B, H * W, C) + e[:, None]).reshape(P, C)}, fb.rowbias_add_ref(x, e, B, H * W, C))["out"]
    r["rowbias_bwd"] = fb.judge({"de": serial(x.reshape(B, H * W, C), 1)}, fb.rowbias_bwd_ref(x, B, H * W, C))["de"]
    return r


@pytest.mark.parametrize("B,H,W,C", IMG)
def test_unet_movement_emulation_inside_bounds(B, H, W, C):
    r = img_ratios(B, H, W, C)
    note("img", r, f"{B}x{H}x{W}x{C}")
    assert all(v <= 1.0 for v in r.values()), r


def block_sum(v):
    """v [.., n] in thread order: thread t adds elements t, t + 256, ...; wave tree; (w0 + w1) + (w2 + w3)"""
    n = v.shape[-1]
    T = -(-n // 256)
    per = serial(Fn.pad(v, (0, T * 256 - n)).reshape(*v.shape[:-1], T, 256), -2)
    w = tree(per.reshape(*v.shape[:-1], 4, 64))
    return (w[..., 0] + w[..., 1]) + (w[..., 2] + w[..., 3])


def emu_gn_stats(x, B, HW, C, G, eps):
    cg = C // G
    n = torch.tensor(float(HW * cg))
    xg = x.reshape(B, HW, G, cg).permute(0, 2, 1, 3).reshape(B, G, HW * cg)
    mu = block_sum(xg) / n
    d = xg - mu[..., None]
    var = block_sum(d * d) / n
    return {"stats": torch.stack([mu, 1.0 / torch.sqrt(var + torch.tensor(eps, dtype=F32))], -1)}


def emu_gn_apply(x, stats, w, b, fs, fh, silu, B, HW, C, G):
    cg = C // G
    mu, rs = (stats[..., i].repeat_interleave(cg, 1)[:, None, :] for i in (0, 1))
    y = (x.reshape(B, HW, C) - mu) * rs * w + b
    if fs is not None:
        y = y * (1.0 + fs[:, None]) + fh[:, None]
    return {"out": (silu32(y) if silu else y).reshape(B * HW, C)}


def emu_gn_bwd(dout, x, stats, w, b, fs, fh, silu, dres, B, HW, C, G, mut=""):
    cg = C // G
    R = max(256 // cg, 1)
    mu, rs = (stats[..., i].repeat_interleave(cg, 1)[:, None, :] for i in (0, 1))
    xh = (x.reshape(B, HW, C) - mu) * rs
    y = xh * w + b
    f1 = (1.0 + fs[:, None]) if fs is not None else torch.ones(1)
    z = y * f1 + (fh[:, None] if fs is not None else 0.0)
    dz = dout.reshape(B, HW, C) * (dsilu32(z) if silu else 1.0)
    dy = dz * f1
    dxh = dy * w

    def lanes(t):  # [B, HW, C] -> per (pixel lane, channel) partial [B, R, C]
        T = -(-HW // R)
        return serial(Fn.pad(t, (0, 0, 0, T * R - HW)).reshape(B, T, R, C), 1)

    def group(t):  # thread (r, cl) = r cg + cl of the group's block -> block sum per (b, g)
        p = lanes(t).reshape(B, R, G, cg).permute(0, 2, 1, 3).reshape(B, G, R * cg)
        return block_sum(Fn.pad(p, (0, 256 - R * cg)))

    n = torch.tensor(float(HW) if mut == "n_hw" else float(HW) * float(cg))
    m1, m2 = (group(t) / n for t in (dxh, dxh * xh))
    m1, m2 = (m.repeat_interleave(cg, 1)[:, None, :] for m in (m1, m2))
    dx = rs * (dxh - m1 - xh * m2)
    if dres is not None:
        dx = dres.reshape(B, HW, C) + dx
    ch = lambda t: serial(lanes(t), 1)  # noqa: E731
    res = {"dx": dx.reshape(B * HW, C), "dw": ch(dy * xh), "db": ch(dy)}
    if fs is not None:
        res.update(dfs=ch(dz * y), dfh=ch(dz))
    return res


GN_SHAPES = [(1, 32, 32), (77, 96, 8), (16, 512, 2), (64, 36, 3), (5, 64, 32)]


def gn_ratios(HW, C, G, cls, flags, mut=""):
    B = 2
    film, silu, use_dres = bool(flags & 1), bool(flags & 2), bool(flags & 4)
    g = torch.Generator().manual_seed(HW * 31 + C + flags)
    n = lambda *s: torch.randn(s, generator=g)  # noqa: E731
    x = gb.make_x(cls, B, HW, C, G, g, "cpu").float().reshape(B * HW, C)
    ref = fb.gn_stats_ref(x, B, HW, C, G, fb.GN_EPS)
    r = fb.judge(emu_gn_stats(x, B, HW, C, G, fb.GN_EPS), ref)
    st = ref["stats"][0].float()
    w, b = 1.0 + 0.2 * n(C), 0.2 * n(C)
    fs, fh = (0.3 * n(B, C), 0.3 * n(B, C)) if film else (None, None)
    r.update(fb.judge(emu_gn_apply(x, st, w, b, fs, fh, silu, B, HW, C, G), fb.gn_apply_ref(x, st, w, b, fs, fh, silu, B, HW, C, G)))
    dout, dres = n(B * HW, C), (n(B * HW, C) if use_dres else None)
    r.update(fb.judge(emu_gn_bwd(dout, x, st, w, b, fs, fh, silu, dres, B, HW, C, G, mut),
                      fb.gn_bwd_ref(dout, x, st, w, b, fs, fh, silu, dres, B, HW, C, G)))
    return r


@pytest.mark.parametrize("HW,C,G", GN_SHAPES)
def test_gn_emulation_inside_bounds(HW, C, G):
    for flags in range(8):
        cls = ("scaled", "offset32", "const")[(GN_SHAPES.index((HW, C, G)) + flags) % 3]
        r = gn_ratios(HW, C, G, cls, flags)
        note("gn", r, f"HW{HW} C{C} G{G} {cls} f{flags}")
        assert all(v <= 1.0 for v in r.values()), (cls, flags, r)


# ------------------------------------------------------------------------------------------------------------------ mutants
MUTANTS = [  # (name, what it plants, thunk -> ratios, outputs of which at least one must leave its bound / bit-compare)
    ("drop_j1", "chunk j = 1 dropped in the row kernel at D = 260", lambda: ln_ratios(260, 13, 3, "scaled", "w", "drop_j1"), ("out", "mean", "rstd")),
    ("mean_n", "mean over 4 ceil(D4 / 64) 64 instead of D", lambda: ln_ratios(260, 13, 3, "scaled", "w", "mean_n"), ("mean", "rstd", "out")),
    ("scale_no1", "1 + scale applied as scale", lambda: ln_ratios(260, 13, 3, "scaled", "w", "scale_no1"), ("out",)),
    ("dres", "dres dropped", lambda: ln_ratios(260, 13, 3, "scaled", "wr", "dres"), ("dx",)),
    ("rot_all", "rotation applied to rot..dh as well", lambda: qk_ratios(2, 64, 32, False, "rot_all"), ("qk",)),
    ("pos_ignored", "pos ignored", lambda: qk_ratios(2, 64, 32, True, "pos_ignored"), ("qk",)),
    ("inv_sign", "the inverse rotation's sign kept", lambda: qk_ratios(2, 64, 64, False, "inv_sign"), ("dqk_in", "dscale")),
    ("drop_last_split", "the last K-split dropped", lambda: gemm_ratios(260, 36, 1040, scratch=64 * 260 * 36, mut="drop_last_split"), ("C",)),
    ("bias_per_split", "bias added once per split", lambda: gemm_ratios(132, 124, 1040, bias=True, scratch=64 * 132 * 124, mut="bias_per_split"), ("C",)),
    ("silu_before_pre", "SiLU applied before pre_out is saved",
     lambda: gemm_ratios(132, 124, 20, bias=True, silu=True, pre=True, mut="silu_before_pre"), ("pre_out",)),
    ("nomax", "softmax without max subtraction on the spike row", lambda: softmax_ratios(4096, "nomax"), ("p",)),
    ("masked_nan", "an all-masked row giving NaN", lambda: keymask_ratios("masked_nan"), ("p",)),
    ("hw_swap", "H and W swapped in the im2col border test at 6 x 10", lambda: img_ratios(2, 6, 10, 5, "hw_swap"), ("im2col",)),
    ("unmirrored", "the col2im tap offset unmirrored", lambda: img_ratios(2, 6, 10, 5, "unmirrored"), ("col2im",)),
    ("n_hw", "n = HW instead of HW Cg in the GN backward", lambda: gn_ratios(64, 36, 3, "scaled", 7, "n_hw"), ("dx",)),
    ("sum2of4", "reduce mode summing 2 of 4 pixels", lambda: img_ratios(2, 6, 10, 5, "sum2of4"), ("resample0",)),
]


@pytest.mark.parametrize("name,what,thunk,outs", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_mutant_leaves_a_bound(name, what, thunk, outs):
    r = thunk()
    verdict = {o: round(r[o], 2) for o in outs}
    print(f"mutant {name} ({what}): |diff| / bound {verdict}")
    assert any(not r[o] <= 1.0 for o in outs), f"mutant {name} passes: {verdict}"


def test_nomax_spike_row_is_the_one_that_fails():
    """the spike row alone rejects the missing max subtraction: exp overflows there"""
    g = torch.Generator().manual_seed(4096)
    s = scores(7, 4096, g)[:1]
    assert fb.judge(emu_softmax_fwd(s, True, mut="nomax"), fb.softmax_fwd_ref(s, True))["p"] > 1.0
    assert fb.judge(emu_softmax_fwd(s, True), fb.softmax_fwd_ref(s, True))["p"] <= 1.0


# ------------------------------------------------------------------------------------------------------------------ references
def test_references_match_fp64_autograd():
    g = torch.Generator().manual_seed(11)
    n = lambda *s: torch.randn(s, generator=g)  # noqa: E731
    # LayerNorm + modulate with the gated residual
    M, D, rpm = 6, 36, 3
    x, w, b, mod, t, dout, dres = n(M, D), n(D), n(D), n(2, 3 * D), n(M, D), n(M, D), n(M, D)
    L = [v.double().requires_grad_(True) for v in (x, w, b, mod, t)]
    xd, wd, bd, md, td = L
    xo = xd + td * md[:, 2 * D:].repeat_interleave(rpm, 0)
    y = Fn.layer_norm(xo, (D,), wd, bd, fb.LN_EPS) * (1.0 + md[:, D:2 * D].repeat_interleave(rpm, 0)) + md[:, :D].repeat_interleave(rpm, 0)
    ((y * dout.double()).sum() + (xo * dres.double()).sum()).backward()
    f = fb.ln_fwd_ref(x, w, b, mod[:, D:2 * D], mod[:, :D], rpm, fb.LN_EPS, t, mod[:, 2 * D:])
    assert float((f["out"][0] - y.detach()).abs().max()) < 1e-9  # (eps enters as its f32 value)
    xin = f["x_out"][0]
    r = fb.ln_bwd_ref(dout, xin, w, b, mod[:, D:2 * D], rpm, f["mean"][0], f["rstd"][0], dres, True, t, mod[:, 2 * D:])
    assert float((r["dx"][0] - xd.grad).abs().max()) < 1e-7
    assert float((r["dscale"][0] - md.grad[:, D:2 * D]).abs().max()) < 1e-7 and float((r["dshift"][0] - md.grad[:, :D]).abs().max()) < 1e-7
    assert float((r["dgate"][0] - md.grad[:, 2 * D:]).abs().max()) < 1e-7 and float((r["dt"][0] - td.grad).abs().max()) < 1e-7
    assert float((r["dwb"][0][:, 0].sum(0) - wd.grad).abs().max()) < 1e-7 and float((r["dwb"][0][:, 1].sum(0) - bd.grad).abs().max()) < 1e-7
    # QK-RMSNorm + RoPE
    B, N, H, dh, rot = 2, 3, 2, 8, 4
    Dq = H * dh
    qkv, sq, sk, dqk = n(B * N, 2 * Dq), n(Dq), n(Dq), n(B * N, 2 * Dq)
    cs, sn = fb.rope_tables(5, rot, g, "cpu")
    tok = torch.tensor([4, 0, 2, 2, 1, 3])
    qd, sqd, skd = (v.double().requires_grad_(True) for v in (qkv, sq, sk))
    outs = []
    for part, scl in ((0, sqd), (1, skd)):
        v = qd[:, part * Dq:(part + 1) * Dq]
        yv = (v * torch.rsqrt(v.square().mean(1, keepdim=True) + fb.f32c(fb.QK_EPS)) * scl).reshape(B * N, H, dh)
        pr = yv[..., :rot].reshape(B * N, H, rot // 2, 2)
        c, s = cs.double()[tok][:, None, :], sn.double()[tok][:, None, :]
        ro = torch.stack([pr[..., 0] * c - pr[..., 1] * s, pr[..., 0] * s + pr[..., 1] * c], -1).reshape(B * N, H, rot)
        outs.append(torch.cat([ro, yv[..., rot:]], -1).reshape(B * N, Dq))
    o = torch.cat(outs, 1)
    (o * dqk.double()).sum().backward()
    f = fb.qk_fwd_ref(qkv, sq, sk, cs, sn, tok, H, dh, rot, fb.QK_EPS)
    assert float((f["qk"][0] - o.detach()).abs().max()) < 1e-12
    r = fb.qk_bwd_ref(dqk, qkv, sq, sk, cs, sn, tok, f["rrms"][0], B, N, H, dh, rot)
    assert float((r["dqk_in"][0] - qd.grad).abs().max()) < 1e-11
    assert float((r["dscale"][0].sum(0) - torch.stack([sqd.grad, skd.grad])).abs().max()) < 1e-11
    # softmax, GEGLU, SwiGLU, DDT conditioning, col2im as the adjoint of im2col
    s, dp = n(5, 9).double().requires_grad_(True), n(5, 9)
    p = torch.softmax(s, -1)
    (p * dp.double()).sum().backward()
    assert float((fb.softmax_bwd_ref(p.detach(), dp, False)["ds"][0] - s.grad).abs().max()) < 1e-12
    u, dh_ = n(4, 6).double().requires_grad_(True), n(4, 3)
    (u[:, :3] * Fn.gelu(u[:, 3:]) * dh_.double()).sum().backward()
    assert float((fb.geglu_bwd_ref(dh_, u.detach(), 3)["du"][0] - u.grad).abs().max()) < 1e-9  # (decimal constants of the source)
    u.grad = None
    (Fn.silu(u[:, :3]) * u[:, 3:] * dh_.double()).sum().backward()
    assert float((fb.swiglu_bwd_ref(dh_, u.detach(), 3)["du"][0] - u.grad).abs().max()) < 1e-12
    enc, temb, dsz = n(6, 4).double().requires_grad_(True), n(2, 4).double().requires_grad_(True), n(6, 4)
    (Fn.silu(Fn.silu(enc + temb.repeat_interleave(3, 0))) * dsz.double()).sum().backward()
    r = fb.ddt_bwd_ref(dsz, enc.detach(), temb.detach(), 3)
    assert float((r["denc"][0] - enc.grad).abs().max()) < 1e-12 and float((r["dtemb"][0] - temb.grad).abs().max()) < 1e-12
    Bc, Hc, Wc, Cc = 2, 3, 5, 2
    xi, dc = n(Bc * Hc * Wc, Cc).double().requires_grad_(True), n(Bc * Hc * Wc, Cc * 9)
    (fb._taps(xi.reshape(Bc, Hc, Wc, Cc)).reshape(-1, Cc * 9) * dc.double()).sum().backward()
    assert float((fb.col2im_ref(dc, Bc, Hc, Wc, Cc)["dx"][0] - xi.grad).abs().max()) < 1e-12
    # im2col against F.unfold (channel-major columns, tap = 3 ky + kx)
    unf = Fn.unfold(xi.detach().reshape(Bc, Hc, Wc, Cc).permute(0, 3, 1, 2), 3, padding=1).permute(0, 2, 1).reshape(-1, Cc * 9)
    assert torch.equal(fb.im2col_ref(xi.detach(), Bc, Hc, Wc, Cc)["cols"][0], unf)
    # GroupNorm statistics and backward
    Bg, HW, C, G = 2, 7, 12, 3
    xg, wg, bg, fsg, fhg, dg = n(Bg * HW, C), n(C), n(C), n(Bg, C), n(Bg, C), n(Bg * HW, C)
    Lg = [v.double().requires_grad_(True) for v in (xg, wg, bg, fsg, fhg)]
    yg = Fn.group_norm(Lg[0].reshape(Bg, HW, C).permute(0, 2, 1), G, Lg[1], Lg[2], fb.f32c(fb.GN_EPS)).permute(0, 2, 1)
    yg = Fn.silu(yg * (1.0 + Lg[3][:, None]) + Lg[4][:, None])
    (yg.reshape(-1, C) * dg.double()).sum().backward()
    st = fb.gn_stats_ref(xg, Bg, HW, C, G, fb.GN_EPS)["stats"][0]
    assert float((fb.gn_apply_ref(xg, st, wg, bg, fsg, fhg, True, Bg, HW, C, G)["out"][0] - yg.detach().reshape(-1, C)).abs().max()) < 1e-11
    r = fb.gn_bwd_ref(dg, xg, st, wg, bg, fsg, fhg, True, None, Bg, HW, C, G)
    assert float((r["dx"][0] - Lg[0].grad).abs().max()) < 1e-10
    for name, leaf, fold in (("dw", Lg[1], True), ("db", Lg[2], True), ("dfs", Lg[3], False), ("dfh", Lg[4], False)):
        got = r[name][0].sum(0) if fold else r[name][0]
        assert float((got - leaf.grad).abs().max()) < 1e-10, name


# ------------------------------------------------------------------------------------------------------------------ coverage, constants
def test_coverage_list_names_every_f32_entry_point():
    """every dl_f32_* declaration of include/diffulab_hip.h appears in the GPU table's coverage list, with tests that exist"""
    text = open(os.path.join(ROOT, "include", "diffulab_hip.h")).read()
    names = set(re.findall(r"DL_API\s+int\s+(dl_f32_\w+)\s*\(", text))
    assert len(names) >= 36 and names == set(fb.COVERAGE), sorted(names ^ set(fb.COVERAGE))
    gpu = open(os.path.join(ROOT, "tests", "test_f32_paths_gpu.py")).read()
    defined = set(re.findall(r"^def (test_\w+)\(", gpu, flags=re.M))
    for name, tests in fb.COVERAGE.items():
        assert tests and set(tests) <= defined, (name, tests)
        assert f'"{name}"' in gpu, name  # (the module calls it by name; its last test asserts the call happened)
    assert "pytest.skip" not in gpu and "mark.skip" not in gpu and "xfail" not in gpu  # no case may be skipped at run time


def test_path_enum_mirror():
    """the GPU module's PATHS mirrors enum DlF32Path by name and order"""
    text = open(os.path.join(ROOT, "diffulab_amd", "csrc", "f32_paths.h")).read()
    body = text[text.index("enum DlF32Path"):text.index("DL_F32_PATH_COUNT")]
    names = re.findall(r"^\s*([A-Z][A-Z0-9_]+)\b", body.split("{", 1)[1], flags=re.M)
    gpu = open(os.path.join(ROOT, "tests", "test_f32_paths_gpu.py")).read()
    listed = re.findall(r'"((?:DL_F32_PATH_NONE|F32_[A-Z0-9_]+))"', gpu[gpu.index("PATHS = ["):gpu.index("REACHED")])
    assert names == listed and len(names) == 10


def test_library_allowances_respect_the_cap():
    for v in (fb.EXP_ULP, fb.ERF_ULP, fb.SIN_ULP, fb.COS_ULP, fb.SQRT_ULP, fb.DIV_ULP):
        assert 1 <= v <= fb.ULP_CAP


def test_report():
    """runs last: the worst |diff| / bound of the unmutated emulations per output"""
    print("\nemulation, worst |diff| / bound: " + "; ".join(f"{o} {r:.3f} ({w})" for o, (r, w) in sorted(REPORT.items())))
    assert REPORT and all(r <= 1.0 for r, _ in REPORT.values())
