"""The attention bounds of tests/attention_bounds.py, checked without a GPU.

A plain torch emulation of the DiT attention kernels' arithmetic -- f32 math, 64-key blocks, online softmax, P rounded to bf16 for the
PV product, l summed from the unrounded p, a bf16 store; the backward recomputing p from lse with p and dS rounded to bf16 -- must
stay inside every bound on each input distribution of the GPU table (tests/test_attn_paths_gpu.py), and each planted mutant must fall
outside a bound on at least one of them.  The maximum |diff| / bound of the faithful emulation is printed per output, so that the
headroom is on record; so is each mutant's.  A mutant listed in UNDETECTABLE is one the module docstring of attention_bounds.py
explains; it is reported, not asserted.
"""

from __future__ import annotations

import math

import pytest
import torch

import attention_bounds as ab

BF = torch.bfloat16
LOG2E = ab.f32(1.4426950408889634)
LN2 = ab.f32(0.6931471805599453)
G, N, DH = 2, 256, 64
SCALE = DH**-0.5
DISTS = ("normal", "unit_rms", "peaked", "masked")
UNDETECTABLE = {"lse_ulp"}


def trunc_bf16(x: torch.Tensor) -> torch.Tensor:
    return (x.float().contiguous().view(torch.int32) & -65536).view(torch.float32)


def rne_bf16(x: torch.Tensor) -> torch.Tensor:
    return x.to(BF).float()


def inputs(dist: str, seed: int = 0):
    g = torch.Generator().manual_seed(seed + DISTS.index(dist))
    q, k, v, do = (torch.randn(G, N, DH, generator=g) for _ in range(4))
    bias = None
    if dist == "unit_rms":  # the QK-norm regime
        q, k = (t / t.square().mean(-1, keepdim=True).sqrt() for t in (q, k))
    if dist == "peaked":  # q x 4 and one dominant key in the last key block: the online-softmax rescale fires late
        q = q * 4
        k[:, N - 40] = q[:, 7] / 4
    if dist == "masked":  # 30 % of the keys masked, and a masked tail that is not a multiple of 64
        keep = torch.rand(G, N, generator=g) > 0.3
        keep[:, N - 37:] = False
        keep[:, 0] = True
        bias = torch.zeros(G, N).masked_fill(~keep, float("-inf"))
    return q.to(BF), k.to(BF), v.to(BF), do.to(BF), bias


def emu_fwd(q, k, v, bias, mutant=None):
    c = ab.f32(SCALE * LOG2E)
    qf, kf, vf = q.float(), k.float(), v.float()
    if mutant == "swap_v":  # two V rows swapped inside one key block
        vf = vf.clone()
        vf[:, [70, 90]] = vf[:, [90, 70]]
    m = torch.full((G, N), -math.inf)
    l = torch.zeros(G, N)
    o = torch.zeros(G, N, DH)
    for kb in range(0, N, 64):
        s = qf @ kf[:, kb:kb + 64].transpose(-1, -2) * c
        if bias is not None:
            s = s + (bias[:, kb:kb + 64] * LOG2E)[:, None, :]
        m_new = torch.maximum(m, s.max(-1).values)
        m_new = torch.where(torch.isinf(m_new), torch.zeros_like(m_new), m_new)
        alpha = torch.exp2(m - m_new)
        p = torch.exp2(s - m_new[..., None])
        l = l * alpha + p.sum(-1)
        pb = trunc_bf16(p) if mutant == "trunc_p" else rne_bf16(p)
        if mutant == "zero_frag" and kb == 128:  # one 32-query x 16-key fragment of P lost
            pb[0, 64:96, 16:32] = 0
        o = o * alpha[..., None] + pb @ vf[:, kb:kb + 64]
        m = m_new
    res = o * (1.0 / l)[..., None]
    out = trunc_bf16(res).to(BF) if mutant == "trunc_store" else res.to(BF)
    lse = (m + torch.log2(l)) * LN2
    if mutant == "lse_ulp":
        lse = lse + 2.0**-20  # one f32 ulp of 8.0
    return out, lse


def emu_bwd(q, k, v, do, out, lse, bias, mutant=None, out_for_delta=None):
    c = ab.f32(SCALE * LOG2E)
    qf, kf, vf, dof = q.float(), k.float(), v.float(), do.float()
    lse2 = lse * LOG2E
    s = qf @ kf.transpose(-1, -2) * c
    if bias is not None:
        s = s + (bias * LOG2E)[:, None, :]
    p = torch.exp2(s - lse2[..., None])
    dp = dof @ vf.transpose(-1, -2)
    o = out.float() if out_for_delta is None else out_for_delta
    delta = (o * dof).sum(-1, keepdim=True)
    ds = p * (dp - delta)
    pb, dsb = rne_bf16(p), rne_bf16(ds)
    mul = 1.0 if mutant == "no_scale" else SCALE
    dq = ((dsb @ kf) * mul).to(BF)
    dk = ((dsb.transpose(-1, -2) @ qf) * SCALE).to(BF)
    dv = (pb.transpose(-1, -2) @ dof).to(BF)
    return dq, dk, dv


def ratios(q, k, v, do, bias, fwd_mutant=None, bwd_mutant=None):
    """max |diff| / bound per output of one emulated forward + backward (the backward on the forward's own out / lse)"""
    out, lse = emu_fwd(q, k, v, bias, fwd_mutant)
    r_out, b_out, r_lse, b_lse = ab.attn_fwd(q, k, v, SCALE, bias)
    res = {"out": _ratio(out, r_out, b_out), "lse": _ratio(lse, r_lse, b_lse)}
    out0, lse0 = emu_fwd(q, k, v, bias) if fwd_mutant else (out, lse)
    kw = {}
    lse_in = lse0
    if bwd_mutant == "delta_fp64":  # delta from the exact out, while the reference is fed the kernel's bf16 out
        kw["out_for_delta"] = r_out.float()
    if bwd_mutant == "lse_ulp":
        lse_in = lse0 + 2.0**-20
    dq, dk, dv = emu_bwd(q, k, v, do, out0, lse_in, bias, bwd_mutant, **kw)
    r_dq, b_dq, r_dk, b_dk, r_dv, b_dv = ab.attn_bwd(q, k, v, do, out0, lse0, SCALE, bias)
    res.update(dq=_ratio(dq, r_dq, b_dq), dk=_ratio(dk, r_dk, b_dk), dv=_ratio(dv, r_dv, b_dv))
    if bias is not None:  # masked keys: exact zeros
        masked = torch.isinf(bias)
        assert float(dk.float()[masked].abs().max()) == 0.0 and float(dv.float()[masked].abs().max()) == 0.0
        assert float(r_dk[masked].abs().max()) == 0.0 and float(r_dv[masked].abs().max()) == 0.0
    return res


def _ratio(got, ref, bound):
    d = (got.double() - ref).abs()
    r = torch.where(d == 0, torch.zeros_like(d), d / bound.clamp_min(1e-300))
    return float(torch.nan_to_num(r, nan=math.inf).max())


@pytest.mark.parametrize("dist", DISTS)
def test_faithful_emulation_stays_inside_every_bound(dist):
    res = ratios(*inputs(dist))
    print(f"\nfaithful emulation, {dist}: " + ", ".join(f"{k} {v:.3f}" for k, v in res.items()))
    assert all(v < 1.0 for v in res.values()), res


# (name, forward mutant, backward mutant)
MUTANTS = [("trunc_p", "trunc_p", None), ("trunc_store", "trunc_store", None), ("zero_frag", "zero_frag", None),
           ("swap_v", "swap_v", None), ("delta_fp64", None, "delta_fp64"), ("lse_ulp", "lse_ulp", "lse_ulp"),
           ("no_scale", None, "no_scale")]


@pytest.mark.parametrize("name,fm,bm", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_mutant_falls_outside_a_bound(name, fm, bm):
    worst = {}
    for dist in DISTS:
        res = ratios(*inputs(dist), fwd_mutant=fm, bwd_mutant=bm)
        worst[dist] = max(res.items(), key=lambda kv: kv[1])
    rejected = [d for d, (_, r) in worst.items() if r > 1.0]
    print(f"\nmutant {name}: " + ", ".join(f"{d}: {o} {r:.3g}" for d, (o, r) in worst.items())
          + (f" -> rejected on {rejected}" if rejected else " -> NOT rejected (see the docstring of attention_bounds.py)"))
    if name in UNDETECTABLE:
        return
    assert rejected, f"mutant {name} stays inside every bound: {worst}"


def test_probs_and_qk_norm_bounds_admit_f32_arithmetic():
    """the UNet (probs) bounds and the fused QK-norm + RoPE bound against a plain f32 evaluation of the same formulas"""
    g = torch.Generator().manual_seed(7)
    q, k, v, do = (torch.randn(3, n, 72, generator=g).to(BF) for n in (33, 77, 77, 33))
    bias = torch.zeros(3, 77).masked_fill(torch.rand(3, 77, generator=g) < 0.3, float("-inf"))
    bias[:, 5] = 0
    scale = ab.f32(72**-0.5)
    s = q.float() @ k.float().transpose(-1, -2) * scale + bias[:, None, :]
    probs = torch.softmax(s, -1)
    for p_round, rnd in ((False, lambda t: t), (True, rne_bf16)):
        out = (rnd(probs) @ v.float()).to(BF)
        rp, bp, ro, bo = ab.probs_fwd(q, k, v, scale, bias, p_round)
        dp = do.float() @ v.float().transpose(-1, -2)
        ds = probs * (dp - (probs * dp).sum(-1, keepdim=True)) * scale
        dq, dk, dv = (rnd(ds) @ k.float()).to(BF), (rnd(ds).transpose(-1, -2) @ q.float()).to(BF), (rnd(probs).transpose(-1, -2) @ do.float()).to(BF)
        rs, bs, rq, bq, rk, bk, rv, bv = ab.probs_bwd(q, k, v, do, probs, scale, p_round)
        res = dict(probs=_ratio(probs, rp, bp), out=_ratio(out, ro, bo), ds=_ratio(ds, rs, bs), dq=_ratio(dq, rq, bq),
                   dk=_ratio(dk, rk, bk), dv=_ratio(dv, rv, bv))
        print(f"\nprobs forms, bf16_p {p_round}: " + ", ".join(f"{k_} {v_:.3f}" for k_, v_ in res.items()))
        assert all(r < 1.0 for r in res.values()), res
        assert float(probs[torch.isinf(bias)[:, None, :].expand_as(probs)].abs().max()) == 0.0
    B, Nt, H, D, rot = 2, 64, 2, 128, 32
    x = torch.randn(B * Nt, D, generator=g).to(BF)
    ssq = x.float().square().sum(1)
    sc = 1 + 0.1 * torch.randn(D, generator=g)
    ang = torch.rand(Nt, rot // 2, generator=g) * 6
    cos, sin = ang.cos(), ang.sin()
    r = torch.rsqrt(ssq * ab.f32(1.0 / D) + 1e-6)
    y = (x.float() * r[:, None] * sc).reshape(B, Nt, H, D // H).clone()
    a, b = y[..., 0:rot:2].clone(), y[..., 1:rot:2].clone()
    y[..., 0:rot:2] = a * cos[None, :, None, :] - b * sin[None, :, None, :]
    y[..., 1:rot:2] = a * sin[None, :, None, :] + b * cos[None, :, None, :]
    ry, by, rr, br = ab.qk_norm_rope(x, ssq, sc, cos, sin, Nt, H, rot, 1e-6)
    res = dict(y=_ratio(y.reshape(B * Nt, D).to(BF), ry, by), r=_ratio(r, rr, br))
    print("\nqk-norm + rope: " + ", ".join(f"{k_} {v_:.3f}" for k_, v_ in res.items()))
    assert all(v_ < 1.0 for v_ in res.values()), res
